// Weight-gradient ("dW") jobs of a backward: which jobs it runs (dw_list), the launches they make — which kernel each goes
// to, how they are split over the points and grouped, and the workspace they need (dw_make_plan, dw_plan.h) — and the
// binding of that plan to pointers and its launch (dw_backward).  The kernels are in dw.hip.h.
#include "dw.hip.h"
#include "dw_plan.h"
#include "rnb_internal.h"

namespace rnb {

// The routing rule.  The one-workgroup-per-gradient kernel (gemm_dw_x3_kernel, or gemm_dw_staged_kernel with
// RNB_VARIANT_DW_STAGED) runs unless RNB_VARIANT_DW_LDS asks for the LDS-staged split-K kernels, and only over whole
// 32-point chunks; then every job of its shape goes to it, and the other jobs to the grouped split-K kernels.
bool dw_one_wg_runs(const Layout& L, int64_t M) {
  return (is_x3(L) || (L.variant & RNB_VARIANT_DW_STAGED) != 0) && !(L.variant & RNB_VARIANT_DW_LDS) && M % kStChunk == 0;
}

// The jobs whose X operand the zero-tile path may leave unwritten — the albedo net's hidden layers and the feature head — all
// go to gemm_dw_x3_kernel, the kernel that honours DwPair::dead.
bool dw_honours_dead(const Layout& L, int64_t M) {
  if (!dw_one_wg_runs(L, M) || !is_x3(L)) return false;
  for (int l = 0; l < L.nc; ++l)
    if (!x3_job_shape(true, L.col[l].Np, L.col[l].Kp)) return false;
  return x3_job_shape(true, L.feat.Np, L.feat.Kp);
}

// One job of dw_list: dW[N x K] (+)= X1^T Y1 (+ X2^T Y2) over the points, with db = the column sums of X of pair
// bias_pair; or, with splits > 0, a reduce-only job: `splits` slabs [N x K] + [N] at part / partb that another kernel
// wrote, summed into dW / db by the reduction launch that follows the last group of weight-gradient jobs.
struct DwListed {
  DwPair p1, p2;
  int npairs, N, K, bias_pair;
  int64_t w_off, b_off;   // dW (leading dimension K) and db: float offsets in the packed gradient
  double flops;
  float* part;
  float* partb;
  int splits;
};

// The weight-gradient jobs of one backward, in the order dw_make_plan takes them: the albedo layers nc-1 .. 0, the reduce-only
// slabs (the fused albedo output layer, the sdf-head row), the feature head, the hidden layers nh-1 .. 0 (with the
// normal two operand pairs: gz_l / u_l and zb_l / in_l; without it the second alone).  On an x2h route the pairs carry
// their maxima slots (h2_slot).  sdfh_slabs > 0: the sdf-head row's gradient waits in pb.sdfh_part as that many slabs.
// Sizing lists a PointBufs without buffers: the operands are then null.
template <class F>
static void dw_list(const Layout& L, const PointBufs& pb, const BwdParts& parts, int sdfh_slabs, F f) {
  const int64_t M = pb.M;
  // the albedo backward's zero-tile path ran: zc_l and cinb of its dead tiles are unwritten (exact zeros); the jobs that take
  // them as X skip those tiles
  const unsigned* dead = parts.dead_dw ? pb.alb_dead : nullptr;
  const unsigned* any_dead = dead != nullptr ? pb.amax + AMAX_ANY_DEAD : nullptr;
  auto job = [&](const DwPair& p1, const DwPair& p2, int npairs, const Lin& ln, int bias_pair, double fl) {
    f(DwListed{p1, p2, npairs, ln.Np, ln.Kp, bias_pair, ln.w_off, ln.b_off, fl, nullptr, nullptr, 0});
  };
  if (parts.albedo) {
    for (int l = L.nc - 1; l >= 0; --l) {
      const float* in = l == 0 ? pb.cin : pb.ac[l - 1];
      const int ldin = l == 0 ? L.Cinp : L.Hcp;
      const DwPair p{pb.zc[l], L.Hcp, in, ldin, 0, h2_slot(L, pb.amax, AMAX_ZC + l),
                     h2_slot(L, pb.smax, l == 0 ? SMAX_CIN : SMAX_AC + l - 1), dead, pb.alb_dead_stride,
                     any_dead};
      job(p, p, 1, L.col[l], 0, mm_flops(M, L.col[l]));
    }
    if (L.route.color == COLOR_H2) {   // the output layer's gradient: per-tile column sums (color_h2_backward)
      const int tiles = (int)(pb.Mp / 64);
      f(DwListed{{}, {}, 0, L.Co, L.Hcp, 0, L.colo.w_off, L.colo.b_off, 0.0, pb.col_part,
                 pb.col_part + (int64_t)tiles * L.Co * L.Hcp, tiles});
    }
  }
  if (!parts.sdf) return;
  if (sdfh_slabs > 0)
    f(DwListed{{}, {}, 0, 1, L.Hp, 0, L.wsdf_off, L.bsdf_off, 0.0, pb.sdfh_part, pb.sdfh_part + (int64_t)sdfh_slabs * L.Hp,
               sdfh_slabs});
  if (parts.feat) {
    const DwPair p{pb.cinb, L.Cinp, pb.a[L.nh - 1], L.Hp, 0, h2_slot(L, pb.amax, AMAX_CINB), h2_slot(L, pb.smax, SMAX_A + L.nh - 1),
                   parts.albedo ? dead : nullptr, pb.alb_dead_stride, any_dead};
    job(p, p, 1, L.feat, 0, mm_flops(M, L.feat));
  }
  for (int l = L.nh - 1; l >= 0; --l) {
    const Lin& ln = L.hid[l];
    const float* in = l == 0 ? pb.e : pb.a[l - 1];
    const int ldin = l == 0 ? L.Ep : L.Hp;
    const float* uin = l == 0 ? pb.geb : pb.u[l];
    // (x2h: adjoint operand, its recorded maximum; the state operand's recorded maximum)
    const DwPair p1{pb.gz[l], L.Hp, uin, ldin, 1, h2_slot(L, pb.amax, AMAX_U + l), h2_slot(L, pb.smax, SMAX_GZ + l)};
    const DwPair p2{pb.zb[l], L.Hp, in, ldin, 0, h2_slot(L, pb.amax, AMAX_ZB + l),
                    h2_slot(L, pb.smax, l == 0 ? SMAX_E : SMAX_A + l - 1)};
    if (parts.normal) job(p1, p2, 2, ln, 1, 2.0 * mm_flops(M, ln));
    else job(p2, p2, 1, ln, 0, mm_flops(M, ln));
  }
}

static DwRouting dw_routing(const Layout& L, int64_t M) {
  return {is_x3(L), L.route.h2, dw_one_wg_runs(L, M), (L.variant & RNB_VARIANT_DW_LDS) != 0, (L.variant & RNB_VARIANT_DETERMINISTIC) != 0};
}
static_assert(kMaxDwListed >= 2 * (RNB_MAX_LIN - 1) + 3, "dw_list: every hidden layer of both networks, two reduce-only jobs, the feature head");

// Lists the jobs of a backward of these parts into `job` and plans them (dw_plan.h).  sizing: the rooms are unbounded;
// else they are the two parts of pb.dw_part as carve_points left them: [0, dw_slab_off) ordered-reduction slabs, the rest
// the one-workgroup kernel's.  A backward of parts the workspace was not carved for gets RNB_E_WORKSPACE from the plan.
static int dw_plan_parts(const Layout& L, const PointBufs& pb, const BwdParts& parts, int sdfh_slabs, bool sizing, DwListed* job,
                         DwPlan* P) {
  DwShape shape[kMaxDwListed];
  int n = 0;
  dw_list(L, pb, parts, sdfh_slabs, [&](const DwListed& j) {
    job[n] = j;
    shape[n++] = DwShape{j.N, j.K, j.npairs};
  });
  const int64_t off = sizing ? 0 : pb.dw_slab_off;
  dw_make_plan(shape, n, pb.M, dw_routing(L, pb.M), sizing ? kDwUnbounded : off, off, sizing ? kDwUnbounded : pb.dw_part_floats - off, P);
  if (P->rc != RNB_OK) RNB_FAIL(P->rc, "%s", P->error);
  return RNB_OK;
}

// Floats of PointBufs::dw_part: the totals of the plan of the render path's jobs (normal on, the colour jobs with_color).
// *slab_off: where the one-workgroup kernel's slabs begin, behind the ordered-reduction slabs of the deterministic variant.
int64_t dw_workspace_floats(const Layout& L, int64_t M, bool with_color, int64_t* slab_off) {
  PointBufs pb{};   // (sizing lists a PointBufs without buffers)
  pb.M = M;
  DwListed job[kMaxDwListed];
  DwPlan P;
  dw_plan_parts(L, pb, BwdParts::render(with_color, false), 0, true, job, &P);   // (the totals do not depend on rc)
  *slab_off = !(L.variant & RNB_VARIANT_DETERMINISTIC) ? 0 : P.det_floats + (is_bf16(L) ? bf16_dw_floats(L, M, with_color) : 0);
  return *slab_off + P.slab_floats;
}

int dw_zero_partials(const Layout& L, const PointBufs& pb, hipStream_t s) {
  if (pb.dw_part == nullptr) RNB_FAIL(RNB_E_WORKSPACE, "no weight-gradient slab workspace was carved");
  if ((L.variant & RNB_VARIANT_DETERMINISTIC) && pb.dw_slab_off > 0)
    RNB_CHECK_HIP(hipMemsetAsync(pb.dw_part, 0, (size_t)pb.dw_slab_off * sizeof(float), s));
  return RNB_OK;
}

// (the cases in the order the kernels have always been instantiated in: the code object lists them in it)
static void dw_launch_kernel(int kernel, dim3 grid, unsigned block, hipStream_t s, const DwGroup& g) {
  switch (kernel) {
    case DW_K_X3_H2: hipLaunchKernelGGL((gemm_dw_x3_kernel<0, 2>), grid, dim3(block), 0, s, g); break;
    case DW_K_X3: hipLaunchKernelGGL((gemm_dw_x3_kernel<0, 3>), grid, dim3(block), 0, s, g); break;
    case DW_K_STAGED: hipLaunchKernelGGL(gemm_dw_staged_kernel<0>, grid, dim3(block), 0, s, g); break;
    case DW_K_REDUCE: hipLaunchKernelGGL(dw_reduce_kernel<0>, grid, dim3(block), 0, s, g); break;
    case DW_K_DIRECT128: hipLaunchKernelGGL((gemm_dw_direct_kernel<128, 3>), grid, dim3(block), 0, s, g); break;
    case DW_K_DIRECT64: hipLaunchKernelGGL((gemm_dw_direct_kernel<64, 3>), grid, dim3(block), 0, s, g); break;
    case DW_K_LDS128: hipLaunchKernelGGL((gemm_dw_kernel<false, 128>), grid, dim3(block), 0, s, g); break;
    case DW_K_LDS64: hipLaunchKernelGGL((gemm_dw_kernel<false, 64>), grid, dim3(block), 0, s, g); break;
    case DW_K_GUARDED: hipLaunchKernelGGL((gemm_dw_kernel<true, 64>), grid, dim3(block), 0, s, g); break;
  }
}

// One launch of the plan: binds the operands, packed_grad + w_off and dw_part + offset into a DwGroup and launches it and
// its slab reduction.
static int dw_launch(const DwLaunch& l, const DwListed* job, const PointBufs& pb, float* packed_grad, hipStream_t s) {
  DwGroup g;
  g.njobs = l.njobs;
  g.M = (int)pb.M;
  double flops = 0.0;
  for (int q = 0; q < l.njobs; ++q) {
    const DwPlanJob& p = l.job[q];
    const DwListed& src = job[p.src];
    DwJob& j = g.job[q];
    j.p1 = src.p1; j.p2 = src.p2;
    j.p1.Y += p.col0; j.p2.Y += p.col0;           // column range of the Y operands (their leading dimension stays)
    j.dW = packed_grad + src.w_off + p.col0;
    j.db = p.col0 == 0 ? packed_grad + src.b_off : nullptr;   // the bias sums (columns of X) belong to the first range
    j.part = p.part < 0 ? nullptr : pb.dw_part + p.part;
    j.partb = p.partb < 0 ? nullptr : pb.dw_part + p.partb;
    j.npairs = p.npairs; j.N = p.N; j.K = p.K; j.lddw = src.K; j.bias_pair = src.bias_pair;
    j.splits = p.splits; j.rows_per_split = p.rows_per_split; j.block_end = p.block_end;
    if (p.col0 + p.K == src.K) flops += src.flops;
  }
  for (int q = l.njobs; q < l.nreduce; ++q) {   // reduce-only jobs: no blocks of the kernel (block_end stays the grid)
    const DwListed& src = job[l.extra[q - l.njobs]];
    DwJob& j = g.job[q];
    memset(&j, 0, sizeof(j));
    j.dW = packed_grad + src.w_off; j.db = packed_grad + src.b_off; j.part = src.part; j.partb = src.partb;
    j.N = src.N; j.K = src.K; j.lddw = src.K; j.splits = src.splits; j.block_end = l.grid;
  }
  // (the one-workgroup kernel and its slab reduction in two scopes: the class time of the weight-gradient kernel is then its
  // own launch duration, as a kernel trace shows it; the ordered reduction of the split-K slabs inside its kernel's)
  const bool one_wg = l.kernel >= DW_K_X3_H2;
  const dim3 reduce((unsigned)256, (unsigned)l.nreduce);
  if (l.grid > 0) {
    ProfScope prof(flops, s, one_wg ? "dW(x3: 256x256 + narrow jobs)" : "dW(other)");
    dw_launch_kernel(l.kernel, dim3((unsigned)l.grid), (unsigned)l.block, s, g);
    RNB_CHECK_LAUNCH();
    if (!one_wg && l.nreduce > 0) dw_launch_kernel(DW_K_REDUCE, reduce, 256, s, g);
  }
  if (one_wg) {
    ProfScope prof(0.0, s, "dW(slab reduce)");
    dw_launch_kernel(DW_K_REDUCE, reduce, 256, s, g);
  }
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// Called after every other launch of the backward: no job reads a buffer that a later launch writes.
int dw_backward(const Layout& L, const PointBufs& pb, const BwdParts& parts, int sdfh_slabs, float* packed_grad, hipStream_t s) {
  DwListed job[kMaxDwListed];
  DwPlan P;
  RNB_TRY(dw_plan_parts(L, pb, parts, sdfh_slabs, false, job, &P));
  for (int i = 0; i < P.nlaunches; ++i) RNB_TRY(dw_launch(P.launch[i], job, pb, packed_grad, s));
  return RNB_OK;
}

}  // namespace rnb
