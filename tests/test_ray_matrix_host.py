"""The table of tests/ray_matrix.py on the host (no GPU): the library's workspace queries accept every accepted row and refuse
every refused row they can see, with a message that names the limit; the oracle resolves every accepted row (shapes, sorted
depths, index range), so the device tests of tests/test_gpu_ray_matrix.py cannot pass against an oracle that mis-shapes; and
the near-tie rule of the up_sample_kernel test holds on the table's own (n, n_new) pairs as an input property."""
import ctypes as C

import pytest
import torch

import rnb_neus_fork_amd as R
from oracle import rnb_oracle as O
from tests import ray_matrix as M
from tests.shape_matrix import BY_NAME as SHAPE_BY_NAME, desc_of, live_params

W32 = SHAPE_BY_NAME["w32"]
SHAPES = [W32, SHAPE_BY_NAME["default_64x64"]]


def _desc(shape, row, **variant):
    d = desc_of(shape.mc, **variant)
    d.n_samples, d.n_importance, d.up_sample_steps = row.n_samples, row.n_importance, row.up_sample_steps
    return d


def _sample_query(shape, row, B=16):
    lib = R.native.load()
    n = C.c_int64(-1)
    rc = lib.rnb_sample_workspace_bytes(C.byref(_desc(shape, row)), B, C.byref(n))
    return rc, n.value, lib.rnb_last_error_string().decode()


def _render_query(shape, row, B=16, flags=None, S=None):
    lib = R.native.load()
    n = C.c_int64(-1)
    flags = R.native.MODE_MVPS if flags is None else flags
    rc = lib.rnb_render_workspace_bytes(C.byref(_desc(shape, row)), B, row.S if S is None else S, flags, C.byref(n))
    return rc, n.value, lib.rnb_last_error_string().decode()


def test_the_table_is_what_it_says():
    names = {r.name for r in M.ACCEPTED}
    for want in ("2+0", "2+2/1", "3+3/3", "5+40/8", "17+5/1", "63+63/1", "64+0", "65+0", "65+64/1", "66+21/3", "100+90/2",
                 "127+64/1", "129+39/3", "191+192/3", "448+64/1", "64+448/7", "256+256/4"):
        assert want in names, want
    for base in ("2+0", "65+64/1"):
        for L in (1, 2, 5, 8):
            assert f"{base}_L{L}" in names
    assert M.BY_NAME["2+0"].S < 64 and M.BY_NAME["65+64/1"].S > 64 and M.BY_NAME["65+64/1"].S % 64 != 0
    r = M.BY_NAME["256+256/4"]
    assert r.n_new == M.K_MAX_NEW and r.step_n[-1] + r.n_new == M.K_MAX_Z and r.S == M.K_MAX_S
    assert M.BY_NAME["64+448/7"].step_n == [64, 128, 192, 256, 320, 384, 448]
    assert M.BY_NAME["3+3/3"].n_new == 1 and M.BY_NAME["5+40/8"].n_new == 5
    for r in M.ACCEPTED:
        assert r.why and 2 <= r.n_samples and r.S <= M.K_MAX_S and r.n_lights <= M.K_MAX_LIGHTS
        assert r.n_new <= min(M.K_MAX_NEW, r.n_samples) and r.n_importance == r.n_new * (r.up_sample_steps if r.n_new else 0)
    for name in M.FUSED_ROW_NAMES + M.BF16_ROW_NAMES:
        assert M.BY_NAME[name].accepted
    pairs = M.up_sample_pairs()
    for want in ((2, 2), (3, 1), (63, 63), (65, 64), (66, 7), (191, 64), (448, 64)):
        assert want in pairs
    assert {len(r.refused_by) > 0 and len(r.limit) > 0 for r in M.REFUSED} == {True}
    assert sorted(M.Z_VALS_S) == [1, 2, 63, 65, 100, 129, 190, 511, 512]


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
@pytest.mark.parametrize("row", M.ACCEPTED, ids=[r.name for r in M.ACCEPTED])
def test_accepted_rows_are_accepted_by_the_queries(shape, row):
    rc, n, err = _sample_query(shape, row)
    assert rc == 0 and n > 0, f"{row.name}: rnb_sample_workspace_bytes refused: {err}"
    for flags in (R.native.MODE_MVPS, R.native.MODE_CORE | R.native.FLAG_FORWARD_ONLY,
                  R.native.MODE_MVPS | R.native.FLAG_INPUT_GRADS):
        rc, n, err = _render_query(shape, row, flags=flags)
        assert rc == 0 and n > 0, f"{row.name}: rnb_render_workspace_bytes refused: {err}"


@pytest.mark.parametrize("S", M.Z_VALS_S)
def test_explicit_sample_counts_are_accepted_by_the_render_query(S):
    rc, n, err = _render_query(W32, M.BY_NAME["2+0"], S=S)
    assert rc == 0 and n > 0, err


REFUSED_BY_QUERY = [r for r in M.REFUSED if r.refused_by != "call"]


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
@pytest.mark.parametrize("row", REFUSED_BY_QUERY, ids=[f"{r.name}:{r.limit}" for r in REFUSED_BY_QUERY])
def test_refused_rows_are_refused_by_the_query(shape, row):
    """the query must say no to what the entry point will refuse (rnb_sample_rays / rnb_render_fwd call the same checks
    before their first launch: api.hip check_sampling_desc, render_setup)"""
    rc, n, err = _sample_query(shape, row) if row.refused_by == "sample_query" else _render_query(shape, row)
    assert rc == -1, f"{row.name}: accepted ({n} bytes): {row.why}"
    assert row.limit in err, f"{row.name}: the message must name the limit {row.limit!r}: {err!r}"
    if row.refused_by == "render_query":   # the neighbour below the limit is fine, in every mode
        assert _render_query(shape, row, S=row.S - 1)[0] == 0
        assert _render_query(shape, row, flags=R.native.MODE_CORE | R.native.FLAG_FORWARD_ONLY)[0] == -1


def test_the_call_only_row_is_invisible_to_the_queries():
    """9 lights: neither query takes a light count, so render_setup refuses it (device test: before any launch)"""
    (row,) = [r for r in M.REFUSED if r.refused_by == "call"]
    assert row.n_lights == M.K_MAX_LIGHTS + 1
    assert _sample_query(W32, row)[0] == 0 and _render_query(W32, row)[0] == 0


@pytest.mark.parametrize("row", M.BASE_ROWS, ids=[r.name for r in M.BASE_ROWS])
def test_oracle_resolves_the_row(row):
    """fp32 oracle on the w32 state of the device tests: z_vals [B, S] sorted, every step's inds in [0, n] and of shape
    [B, n_new], the initial depths the odd-n linspace, the render's outputs of the row's shapes"""
    mc = O.ModelConf(sdf=W32.mc.sdf, color=W32.mc.color, render=row.render_conf)
    p = live_params(mc, W32.seed)
    B = 16
    b = O.synthetic_batch(B, n_lights=row.n_lights, seed=11, step=1, warmup=False)
    tr = {}
    with torch.no_grad():
        out = O.render_rnb(p, mc, b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                           t_rand=b["t_rand"], trace=tr)
    z = out["z_vals"]
    assert z.shape == (B, row.S)
    assert bool((z[:, 1:] >= z[:, :-1]).all()), "depths must be sorted"
    assert out["color_fine"].shape == (row.n_lights, B, 3) and out["weights"].shape == (B, row.S)
    steps = tr.get("steps", [])
    assert [st["z_in"].shape[1] for st in steps] == row.step_n
    for st, n in zip(steps, row.step_n):
        assert st["inds"].shape == (B, row.n_new) and st["new_z"].shape == (B, row.n_new)
        assert int(st["inds"].min()) >= 0 and int(st["inds"].max()) <= n
        assert st["cdf"].shape == (B, n) and bool((st["cdf"][:, 1:] >= st["cdf"][:, :-1]).all())
        assert st["sort_index"].shape == (B, n + row.n_new)
        assert torch.equal(torch.sort(st["sort_index"], dim=1).values, torch.arange(n + row.n_new).expand(B, -1))
    z0 = steps[0]["z_in"] if steps else z
    lin = torch.linspace(0.0, 1.0, row.n_samples)
    assert torch.equal(z0, b["near"] + (b["far"] - b["near"]) * lin[None, :] + (b["t_rand"] - 0.5) * 2.0 / row.n_samples)


def test_near_tie_rule_on_the_tables_pairs():
    """The input property the device test relies on (tests/test_gpu_ray_matrix.py): with cdf' the fp32 oracle re-expressed
    the way the kernel differs from PyTorch (sigmoid as 1 / (1 + exp(-x)), normaliser summed sequentially in double), a
    sample is exempt from the exact-index check when a cdf value lies within 2 max|cdf - cdf'| of its u.  Exempt samples
    are <= max(1, 0.1 %) of every case and <= 0.02 % of all, and the re-expressed oracle itself changes no unexempt index."""
    total = exempt_all = 0
    worst = 0.0
    for n, n_new in M.up_sample_pairs():
        for inv_s in M.UP_INV_S:
            r = M.up_sample_reference(n, n_new, inv_s)
            assert r["inds"].shape == (M.UP_RAYS, n_new) and r["cdf"].shape == (M.UP_RAYS, n)
            assert bool((r["z"][:, 1:] >= r["z"][:, :-1]).all()), "input depths must be sorted"
            cdf2 = M.up_sample_cdf_reexpressed(r["rays_o"], r["rays_d"], r["z"], r["sdf"], inv_s)
            exempt, margin = M.near_tie_exempt(r["cdf"], cdf2, n_new)
            worst = max(worst, margin / 2.0)
            u = torch.linspace(0.5 / n_new, 1.0 - 0.5 / n_new, steps=n_new).expand(M.UP_RAYS, n_new).contiguous()
            inds2 = torch.searchsorted(cdf2.contiguous(), u, right=True)
            flipped = int(((inds2 != r["inds"]) & ~exempt).sum())
            k = int(exempt.sum())
            assert k <= max(1.0, 1e-3 * exempt.numel()), f"n={n} n_new={n_new} inv_s={inv_s}: {k} near ties: a bad input"
            assert flipped == 0, f"n={n} n_new={n_new} inv_s={inv_s}: the re-expressed oracle flips {flipped} unexempt indices"
            total += exempt.numel()
            exempt_all += k
    print(f"near ties: {exempt_all} exempt of {total} samples; max |cdf - cdf'| {worst:.2e}")
    assert exempt_all <= 2e-4 * total


def _linspace_at(n, split):
    """rnb_internal.h linspace_at(0, 1, n, i) for every i in exact fp32 (a double holds the fused multiply-add's exact
    result), with the halves split at `split`"""
    step = (torch.tensor(1.0) / torch.tensor(float(n - 1))).double()
    i = torch.arange(n, dtype=torch.float64)
    return torch.where(i < split, step * i, 1.0 - step * (n - 1 - i)).float()


def test_linspace_restatement_and_what_its_split_decides():
    """torch.linspace(0, 1, n) is start + step i on the first n // 2 elements and end - step (n - 1 - i) on the rest, each one
    fused multiply-add — for every n the sampler accepts.  The device test compares z_init_kernel with torch.linspace on the
    unit interval over the same n; moving the split to (n + 1) // 2 changes a value at 79 odd n, so that test sees it."""
    moved = []
    for n in range(2, M.K_MAX_S + 1):
        assert torch.equal(_linspace_at(n, n // 2), torch.linspace(0.0, 1.0, n)), n
        if not torch.equal(_linspace_at(n, (n + 1) // 2), _linspace_at(n, n // 2)):
            moved.append(n)
    assert len(moved) == 79 and all(n % 2 == 1 for n in moved) and 127 in moved and 191 in moved
