"""Render gradients with respect to the inputs (rays_o, rays_d, lights_dir, background_rgb, near / far / z_vals) against
fp64 torch autograd through oracle/rnb_oracle.py, plus their contracts: frozen networks, additivity with the parameter
gradients, bit-reproducibility, the bf16 refusal and the data-parallel shard rule.

The oracle's sdf_gradient detaches its input; the reference's gradient() (models/fields.py:114-127) keeps the graph to the
points when they require grad, so the normal's Hessian-vector term is part of the reference's ray gradient.  Every oracle
call here runs with a graph-keeping normal (the graph_normal fixture of tests/oracle_normal.py)."""
import os
from dataclasses import replace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import rnb_oracle as O
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device, explicit_depths, free_port
from tests.oracle_normal import graph_normal  # noqa: F401
from tests.parity import check_grad, check_value, grad_bound, rel_l2
from tests.ray_matrix import FLOAT_OUTS, Z_GRAD_S
from tests.shape_matrix import BY_NAME, live_params, step_batch

pytestmark = pytest.mark.gpu

B = 64
SHAPES = ["default_64x64", "feat128", "scale3"]


def _build(R, name, render=None):
    shape = BY_NAME[name]
    mc = shape.mc if render is None else replace(shape.mc, render=render)
    p = live_params(mc, shape.seed)
    sdf, devn, col, ren = R.build_from_named_params(mc, p, device())
    return mc, p, sdf, devn, col, ren


def _functional(out, seed=5):
    """A fixed random linear functional of every float output (scaled to O(1) per tensor)."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    for k in FLOAT_OUTS:
        t = out[k]
        w = torch.randn(tuple(t.shape), generator=g, dtype=torch.float64) / max(1, t.numel()) ** 0.5
        total = total + (w.to(t.device, t.dtype) * t).sum()
    return total


def _loss(out, b, mvps):
    true_rgb = b["true_rgb"] if mvps else b["true_rgb"][:1]
    return _functional(out) + O.rnb_loss(out, true_rgb, b["mask"])[0]


def _case_inputs(case, batch):
    """(inputs dict on the CPU, names of those that require grad)"""
    b = dict(batch)
    if case == "render":
        b["bg"] = torch.tensor([0.2, 0.5, 0.8])
        return b, ("rays_o", "rays_d", "bg")
    if case == "warmup":
        b["lights_dir"] = O.synthetic_batch(B, seed=11, step=1, warmup=True)["lights_dir"]   # shared [L,1,1,3]
    return b, ("rays_o", "rays_d", "lights_dir")


def _native(ren, case, b, want, variant=None):
    ren.set_variant(**(variant or {}))
    for q in ren.sdf_network.parameters():
        q.grad = None
    for q in list(ren.color_network.parameters()) + list(ren.deviation_network.parameters()):
        q.grad = None
    x = {k: v.to(device()).detach().requires_grad_(k in want) for k, v in b.items()}
    zv = x.get("z_vals")     # explicit depths (an input like the others: it may require grad), else the device samples
    if case == "render":
        out = ren.render(x["rays_o"], x["rays_d"], x["near"], x["far"], background_rgb=x["bg"], cos_anneal_ratio=0.5,
                         t_rand=x["t_rand"], z_vals=zv)
    else:
        fn = ren.render_rnb_warmup if case == "warmup" else ren.render_rnb
        out = fn(x["rays_o"], x["rays_d"], x["near"], x["far"], x["lights_dir"], cos_anneal_ratio=0.5, t_rand=x["t_rand"],
                 z_vals=zv)
    _loss(out, x, case != "render").backward()
    torch.cuda.synchronize()
    return out, {k: x[k].grad for k in want}


def _oracle(p, mc, case, b, want, z, dt, outs=None):
    """`z`: the depths the device sampled, or None with explicit depths in b["z_vals"]; `outs`: receives the outputs"""
    q = {k: v.to(dt).detach().requires_grad_(True) for k, v in p.items()}
    x = {k: v.to(dt).detach().requires_grad_(k in want) for k, v in b.items()}
    zv = x["z_vals"] if "z_vals" in x else (None if z is None else z.to(dt))
    with torch.enable_grad():
        if case == "render":
            out = O.render(q, mc, x["rays_o"], x["rays_d"], x["near"], x["far"], background_rgb=x["bg"],
                           cos_anneal_ratio=0.5, z_vals=zv, t_rand=x["t_rand"])
        else:
            out = O.render_rnb(q, mc, x["rays_o"], x["rays_d"], x["near"], x["far"], x["lights_dir"], cos_anneal_ratio=0.5,
                               warmup=case == "warmup", z_vals=zv, t_rand=x["t_rand"])
        _loss(out, x, case != "render").backward()
    if outs is not None:
        outs.update({k: v.detach() for k, v in out.items()})
    return {k: x[k].grad for k in want}


def _check(mine, g64, g32, tag):
    for k in g64:
        assert mine[k] is not None, f"{tag} {k}: no gradient"
        assert bool(torch.isfinite(mine[k]).all()), f"{tag} {k}: not finite"
        assert float(g64[k].norm()) > 0.0, f"{tag} {k}: the fp64 gradient vanishes: not a parity target"
        rel32 = rel_l2(g32[k], g64[k])
        print(f"{tag} {k}: rel-L2 {rel_l2(mine[k].cpu(), g64[k]):.2e} (bound {grad_bound(rel32):.2e})")
        check_grad(f"{tag} {k}", mine[k].cpu(), g64[k], rel32)


# ------------------------------------------------------------------------------------------------------------ case 1
@pytest.mark.parametrize("case", ["render", "rnb", "warmup"])
@pytest.mark.parametrize("name", SHAPES)
def test_input_gradients_against_fp64(R, graph_normal, name, case):
    mc, p, sdf, devn, col, ren = _build(R, name)
    b, want = _case_inputs(case, step_batch(B))
    out, mine = _native(ren, case, b, want)
    assert out["color_fine"].grad_fn is not None
    z = ren.last_z_vals.cpu()
    torch.set_num_threads(16)
    g64 = _oracle(p, mc, case, b, want, z, torch.float64)
    g32 = _oracle(p, mc, case, b, want, z, torch.float32)
    _check(mine, g64, g32, f"{name}/{case}")


# ------------------------------------------------------------------------------------------------------------ case 2
def test_near_far_with_no_importance_samples(R, graph_normal):
    rc = O.RenderConf(n_samples=32, n_importance=0)
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64", render=rc)
    b = step_batch(B)
    want = ("rays_o", "rays_d", "near", "far")

    def native():
        x = {k: v.to(device()).detach().requires_grad_(k in ("rays_o", "rays_d", "lights_dir")) for k, v in b.items()}
        near, far = O.near_far_from_sphere(x["rays_o"], x["rays_d"])
        near.retain_grad()
        far.retain_grad()
        out = ren.render_rnb(x["rays_o"], x["rays_d"], near, far, x["lights_dir"], cos_anneal_ratio=0.5, t_rand=x["t_rand"])
        _loss(out, x, True).backward()
        torch.cuda.synchronize()
        return {"rays_o": x["rays_o"].grad, "rays_d": x["rays_d"].grad, "near": near.grad, "far": far.grad}

    def oracle(dt):
        q = {k: v.to(dt).detach().requires_grad_(True) for k, v in p.items()}
        x = {k: v.to(dt).detach().requires_grad_(k in ("rays_o", "rays_d")) for k, v in b.items()}
        with torch.enable_grad():
            near, far = O.near_far_from_sphere(x["rays_o"], x["rays_d"])
            near.retain_grad()
            far.retain_grad()
            out = O.render_rnb(q, mc, x["rays_o"], x["rays_d"], near, far, x["lights_dir"], cos_anneal_ratio=0.5,
                               t_rand=x["t_rand"])
            _loss(out, x, True).backward()
        return {"rays_o": x["rays_o"].grad, "rays_d": x["rays_d"].grad, "near": near.grad, "far": far.grad}

    mine = native()
    torch.set_num_threads(16)
    _check(mine, oracle(torch.float64), oracle(torch.float32), "n_importance0")
    assert set(mine) == set(want)


# ------------------------------------------------------------------------------------------------------------ case 2b
# Explicit depths that require grad (renderer.py: "z_vals given"): ray_input_adjoint_kernel's z_bar stencil,
#   z_bar_s = mbar_s - [s < S-1] Dbar_s + [s > 0] Dbar_{s-1},
# walks the ray in 64-sample chunks and hands Dbar of a chunk's last sample to the next chunk in carry_D.  S = 2 and 63 stay
# inside one chunk; 65, 129 and 190 carry once or twice into a ragged last chunk (tests/ray_matrix.py Z_GRAD_S).
BZ = 32


def _check_chunk_boundaries(mine, g64, g32, S, tag):
    """the samples on either side of every 64-sample chunk boundary, as a tensor of their own: what carry_D feeds"""
    cols = [c for j0 in range(64, S, 64) for c in (j0 - 1, j0)]
    if cols:
        _check({"z_vals": mine["z_vals"][:, cols]}, {"z_vals": g64["z_vals"][:, cols]}, {"z_vals": g32["z_vals"][:, cols]},
               f"{tag} columns {cols}")


@pytest.mark.parametrize("case", ["render", "rnb"])
@pytest.mark.parametrize("S", Z_GRAD_S)
def test_explicit_depth_gradients_against_fp64(R, graph_normal, S, case):
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64")
    b, want = _case_inputs(case, step_batch(BZ))
    b["z_vals"] = explicit_depths(b, S, seed=7919 * S)
    want = want + ("z_vals",)
    out, mine = _native(ren, case, b, want)
    assert tuple(mine["z_vals"].shape) == (BZ, S)
    assert torch.equal(ren.last_z_vals.cpu(), b["z_vals"]), "the render must run at the depths it was given"
    torch.set_num_threads(16)
    g64 = _oracle(p, mc, case, b, want, None, torch.float64)
    g32 = _oracle(p, mc, case, b, want, None, torch.float32)
    _check(mine, g64, g32, f"z_vals S={S}/{case}")
    _check_chunk_boundaries(mine, g64, g32, S, f"z_vals S={S}/{case}")


@pytest.mark.parametrize("per_ray", [False, True], ids=["shared", "per_ray"])
@pytest.mark.parametrize("L", [1, 2, 5, 8])
def test_light_counts_at_a_carry_and_a_ragged_chunk(R, graph_normal, L, per_ray):
    """1, 2, 5 and kMaxRenderLights = 8 lights at S = 129 explicit depths, shared [L,1,1,3] and per ray [L,B,1,3]:
    lights_dir.grad (with rays and z_vals) by the gradient rule, color_fine per light by the output rule of tests/parity.py"""
    S = 129
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64")
    b = dict(O.synthetic_batch(BZ, n_lights=L, seed=11, step=1, warmup=False))
    if not per_ray:
        gen = torch.Generator().manual_seed(40 + L)
        lt = torch.randn(L, 1, 1, 3, generator=gen)
        b["lights_dir"] = (lt / lt.norm(dim=-1, keepdim=True)).contiguous()
    b["z_vals"] = explicit_depths(b, S, seed=7919 * S)
    want = ("rays_o", "rays_d", "lights_dir", "z_vals")
    out, mine = _native(ren, "rnb", b, want)
    assert tuple(out["color_fine"].shape) == (L, BZ, 3) and tuple(mine["lights_dir"].shape) == tuple(b["lights_dir"].shape)
    torch.set_num_threads(16)
    o64, o32 = {}, {}
    g64 = _oracle(p, mc, "rnb", b, want, None, torch.float64, o64)
    g32 = _oracle(p, mc, "rnb", b, want, None, torch.float32, o32)
    tag = f"{L} lights {'per ray' if per_ray else 'shared'} S={S}"
    _check(mine, g64, g32, tag)
    _check_chunk_boundaries(mine, g64, g32, S, tag)
    for l in range(L):
        r64 = o64["color_fine"][l]
        assert float(r64.abs().max()) > 1e-3, f"{tag}: light {l} renders nothing"
        check_value(f"{tag}: color_fine[{l}]", out["color_fine"][l], r64, o32["color_fine"][l])


# ------------------------------------------------------------------------------------------------------------ cases 3-5
def test_frozen_networks_still_give_ray_gradients(R):
    mc, p, sdf, devn, col, ren = _build(R, "scale3")
    b, want = _case_inputs("rnb", step_batch(B))
    _, ref = _native(ren, "rnb", b, want)
    for net in (sdf, devn, col):
        for q in net.parameters():
            q.requires_grad_(False)
    out, mine = _native(ren, "rnb", b, want)
    assert out["color_fine"].grad_fn is not None and out["weights"].grad_fn is not None
    for k in want:
        assert torch.equal(mine[k], ref[k]), f"frozen networks: {k} differs"
    assert all(q.grad is None for net in (sdf, devn, col) for q in net.parameters())


def _param_grads(ren):
    nets = (ren.sdf_network, ren.deviation_network, ren.color_network)
    return [q.grad.clone() for net in nets for q in net.parameters()]


# (the per-layer albedo path's weight gradients use fp32 atomics in the default variant: compared in the deterministic one)
@pytest.mark.parametrize("name,variant", [("default_64x64", None), ("feat128", dict(deterministic=True))])
def test_parameter_gradients_do_not_change_when_inputs_want_gradients(R, name, variant):
    mc, p, sdf, devn, col, ren = _build(R, name)
    for case in ("render", "rnb"):
        b, want = _case_inputs(case, step_batch(B))
        _native(ren, case, b, (), variant)
        plain = _param_grads(ren)
        _native(ren, case, b, want, variant)
        with_inputs = _param_grads(ren)
        assert all(torch.equal(a, c) for a, c in zip(plain, with_inputs)), f"{name}/{case}: parameter gradients changed"


@pytest.mark.parametrize("variant", [None, dict(deterministic=True)])
def test_input_gradients_are_bit_reproducible(R, variant):
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64")
    for case in ("render", "warmup"):
        b, want = _case_inputs(case, step_batch(B))
        _, g1 = _native(ren, case, b, want, variant)
        _, g2 = _native(ren, case, b, want, variant)
        for k in want:
            assert torch.equal(g1[k], g2[k]), f"{case} {variant}: {k} is not bit-reproducible"


# ------------------------------------------------------------------------------------------------------------ case 6
def test_bf16_refuses_input_gradients_before_any_launch(R):
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64")
    ren.set_variant(bf16=True)
    b = {k: v.to(device()) for k, v in step_batch(B).items()}
    ren.last_z_vals = None
    with pytest.raises(RuntimeError, match="bf16.*no input adjoints"):
        ren.render_rnb(b["rays_o"].requires_grad_(True), b["rays_d"], b["near"], b["far"], b["lights_dir"],
                       t_rand=b["t_rand"])
    assert ren.last_z_vals is None, "the refusal must come before the sampling launches"
    # without an input that requires grad the bf16 variant renders as before
    out = ren.render_rnb(b["rays_o"].detach(), b["rays_d"], b["near"], b["far"], b["lights_dir"], t_rand=b["t_rand"])
    assert bool(torch.isfinite(out["color_fine"]).all())


# ------------------------------------------------------------------------------------------------------------ case 7
def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import rnb_neus_fork_amd as R
    from rnb_neus_fork_amd import parallel as P
    mc = O.ModelConf(sdf=O.SDFConf(d_out=65, d_hidden=64), color=O.ColorConf(d_feature=64, d_hidden=64),
                     render=O.RenderConf(n_samples=16, n_importance=16))
    torch.manual_seed(0)
    p = O.init_params(mc)
    sdf, devn, col, ren = R.build_from_named_params(mc, p, dev)
    ren.set_variant(deterministic=True)
    batch = O.synthetic_batch(24, seed=9, step=2, warmup=True)     # shared lights [L,1,1,3]
    batch["mask"][:9] = 1.0
    batch["mask"][9:] = (torch.arange(15) % 4 == 0).float()[:, None]

    def run(b, dp, group):
        ren.set_data_parallel(enabled=dp, exact=True)
        x = {k: v.to(dev).detach().requires_grad_(k in ("rays_o", "rays_d", "lights_dir")) for k, v in b.items()}
        out = ren.render_rnb_warmup(x["rays_o"], x["rays_d"], x["near"], x["far"], x["lights_dir"], cos_anneal_ratio=1.0,
                                    t_rand=x["t_rand"])
        R.rnb_loss(out, x["true_rgb"], x["mask"], group=group)[0].backward()
        torch.cuda.synchronize()
        return [x[k].grad.cpu() for k in ("rays_o", "rays_d", "lights_dir")]

    single = run(batch, False, None)
    shard = run(P.shard_batch(batch, rank, world), True, dist.group.WORLD)
    lights = shard[2].clone()
    dist.all_reduce(lights)
    lo = rank * 12
    res = (rank, float((shard[0] - single[0][lo:lo + 12]).abs().max() / single[0].abs().max()),
           float((shard[1] - single[1][lo:lo + 12]).abs().max() / single[1].abs().max()),
           float((lights - single[2]).abs().max() / single[2].abs().max()))
    q.put(res)
    dist.destroy_process_group()


def test_data_parallel_input_gradients_are_shard_local(R):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for pr in procs:
        pr.join(timeout=60)
    for rank, d_o, d_d, d_l in res:
        assert d_o <= 1e-5 and d_d <= 1e-5, f"rank {rank}: ray gradients differ from the single-process rows ({d_o:.2e}, {d_d:.2e})"
        assert d_l <= 1e-5, f"rank {rank}: the sum over ranks of the light gradients differs from the single process ({d_l:.2e})"
