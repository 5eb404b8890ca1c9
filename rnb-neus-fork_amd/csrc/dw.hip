// Weight-gradient ("dW") jobs of a backward: which jobs it runs (dw_list), which kernel each goes to (dw_one_wg), how
// they are split over the points and grouped into launches (DwBatch), and the workspace they need (dw_workspace_floats).
// The kernels are in dw.hip.h.
#include "dw.hip.h"
#include "rnb_internal.h"

namespace rnb {

// split-K plan of one dW job: kernel variant v ([0] K % 128 == 0, [1] K % 64 == 0, [2] anything: guarded), number of
// point splits and points per split.  Shared by DwBatch::add and by the sizing of the deterministic partial slabs.
static void dw_plan(int64_t M, int N, int K, int* v_out, int* splits_out, int* rows_out) {
  const bool exact = N % 128 == 0 && M % BK == 0;
  const int v = (exact && K % 128 == 0) ? 0 : (exact && K % 64 == 0) ? 1 : 2;
  const int kt = v == 0 ? 128 : 64;                  // tile width along K of the variant (see kernel)
  const int min_rows = v == 0 ? 1024 : 512;          // points per block (half-size tiles: half the rows)
  const int tiles = ((N + 127) / 128) * ((K + kt - 1) / kt);
  int splits = (int)((M + min_rows - 1) / min_rows);
  const int max_splits = (1024 + tiles - 1) / tiles;  // ~1024 blocks per job
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  if (splits >= 8) splits = splits / 8 * 8;   // multiple of 8: enables the XCD-aware placement in the kernel
  int rows = (int)((M + splits - 1) / splits);
  rows = (rows + BK - 1) / BK * BK;
  // (the kernel tolerates empty splits, so the job keeps the multiple-of-8 split count)
  if ((int64_t)rows * splits < M) splits = (int)((M + rows - 1) / rows);
  *v_out = v;
  *splits_out = splits;
  *rows_out = rows;
}

// Point split of the staged 256 x 256 kernel: one workgroup per (job, split) and ONE round of workgroups (<= 256, one per
// CU), each job's share of them proportional to its work (operand pairs), so every CU multiplies for the whole launch.
// Partial gradients leave through plain stores into slabs that dw_reduce_kernel sums in split order: an fp32 atomic tail
// of 256 KB per workgroup would cost ~50 us per round at the chip's ~1.3 TB/s atomic rate, with nothing to hide under.
// (Restated in Python, with flush_staged's room clamp, by tests/point_matrix.py: a change here changes that table's rows.)
static void dw_staged_plan(int64_t M, int npairs, int total_pairs, int* splits_out, int* rows_out) {
  int splits = total_pairs > 0 ? (256 * npairs) / total_pairs : 1;
  if (splits < 1) splits = 1;
  int64_t rows = (M + splits - 1) / splits;
  rows = (rows + kStChunk - 1) / kStChunk * kStChunk;
  if (rows < 2 * kStChunk) rows = 2 * kStChunk;
  splits = (int)((M + rows - 1) / rows);     // every split is non-empty: the reduction reads every slab
  *splits_out = splits;
  *rows_out = (int)rows;
}

// Jobs of the one-workgroup-per-gradient kernels.  The LDS-DMA staged kernel takes 256 x 256 matrices only; the x3
// kernel also takes 256 x K with K a multiple of 64 as COLUMN RANGES of the Y operand: 256-column ranges run as whole
// jobs, what is left as narrow (64-column) jobs — the PE-input layer (K = 64) and the albedo net's first layer
// (K = 320 = 256 + 64) then ride in the same launch instead of a separate fp32-MFMA one.  Work units for the split
// plan: a 256-column pair costs about twice a narrow pair (a quarter of the MFMAs, the same staging of X).
static bool x3_job_shape(bool x3, int N, int K) { return N == 256 && (K == 256 || (x3 && K % 64 == 0 && K >= 64 && K <= 1024)); }
static int x3_job_units(int npairs, int width) { return npairs * (width >= 256 ? 2 : 1); }
template <class F>
static void x3_for_each_range(int K, F f) {   // f(first column, width): 256-wide ranges, then 64-wide ones
  int c = 0;
  for (; c + 256 <= K; c += 256) f(c, 256);
  for (; c + 64 <= K; c += 64) f(c, 64);
}

// The routing rule.  The one-workgroup-per-gradient kernel (gemm_dw_x3_kernel, or gemm_dw_staged_kernel with
// RNB_VARIANT_DW_STAGED) runs unless RNB_VARIANT_DW_LDS asks for the LDS-staged split-K kernels, and only over whole
// 32-point chunks; then every job of its shape goes to it, and the other jobs to the grouped split-K kernels.
bool dw_one_wg_runs(const Layout& L, int64_t M) {
  return (is_x3(L) || (L.variant & RNB_VARIANT_DW_STAGED) != 0) && !(L.variant & RNB_VARIANT_DW_LDS) && M % kStChunk == 0;
}
static bool dw_one_wg(const Layout& L, int64_t M, int N, int K) { return x3_job_shape(is_x3(L), N, K) && dw_one_wg_runs(L, M); }

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

// The weight-gradient jobs of one backward, in the order DwBatch takes them: the albedo layers nc-1 .. 0, the reduce-only
// slabs (the fused albedo output layer, the sdf-head row), the feature head, the hidden layers nh-1 .. 0 (with the
// normal two operand pairs: gz_l / u_l and zb_l / in_l; without it the second alone).  On an x2h route the pairs carry
// their maxima slots (h2_slot).  sdfh_slabs > 0: the sdf-head row's gradient waits in pb.sdfh_part as that many slabs.
// Sizing lists a PointBufs without buffers: the operands are then null.
template <class F>
static void dw_list(const Layout& L, const PointBufs& pb, const BwdParts& parts, int sdfh_slabs, F f) {
  const int64_t M = pb.M;
  auto job = [&](const DwPair& p1, const DwPair& p2, int npairs, const Lin& ln, int bias_pair, double fl) {
    f(DwListed{p1, p2, npairs, ln.Np, ln.Kp, bias_pair, ln.w_off, ln.b_off, fl, nullptr, nullptr, 0});
  };
  if (parts.albedo) {
    for (int l = L.nc - 1; l >= 0; --l) {
      const float* in = l == 0 ? pb.cin : pb.ac[l - 1];
      const int ldin = l == 0 ? L.Cinp : L.Hcp;
      const DwPair p{pb.zc[l], L.Hcp, in, ldin, 0, h2_slot(L, pb.amax, AMAX_ZC + l),
                     h2_slot(L, pb.smax, l == 0 ? SMAX_CIN : SMAX_AC + l - 1)};
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
    const DwPair p{pb.cinb, L.Cinp, pb.a[L.nh - 1], L.Hp, 0, h2_slot(L, pb.amax, AMAX_CINB), h2_slot(L, pb.smax, SMAX_A + L.nh - 1)};
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

// The two parts of PointBufs::dw_part: [ordered-reduction slabs of the split-K kernels | slabs of the one-workgroup
// kernel], sized for the render path's jobs (normal on, the colour jobs with_color); the slabs for every job of the
// one-workgroup kernel's shape, whether the variant routes it there or not.  A backward with fewer operand pairs per job
// splits finer and is held to the room by DwBatch::flush_staged.
static void dw_sizes(const Layout& L, int64_t M, bool with_color, int64_t* det_floats, int64_t* staged_floats) {
  PointBufs pb{};
  pb.M = M;
  const bool x3 = is_x3(L);
  // (reduce-only jobs are other kernels' slabs, carved with their producers: no room of their own here)
  auto each_job = [&](auto f) {
    dw_list(L, pb, BwdParts::render(with_color, false), 0, [&](const DwListed& j) { if (j.npairs > 0) f(j); });
  };
  int total_units = 0;
  each_job([&](const DwListed& j) {
    if (x3_job_shape(x3, j.N, j.K)) x3_for_each_range(j.K, [&](int, int width) { total_units += x3_job_units(j.npairs, width); });
  });
  *det_floats = *staged_floats = 0;
  each_job([&](const DwListed& j) {
    int splits, rows;
    if (x3_job_shape(x3, j.N, j.K))
      x3_for_each_range(j.K, [&](int, int width) {
        dw_staged_plan(M, x3_job_units(j.npairs, width), total_units, &splits, &rows);
        *staged_floats += (int64_t)splits * j.N * width + (int64_t)splits * j.N;
      });
    // (jobs of the one-workgroup kernel leave through its own slabs, whatever the variant: no ordered-reduction slabs —
    // and no 200 MB memset per step — for them)
    if (!dw_one_wg(L, M, j.N, j.K)) {
      int v;
      dw_plan(M, j.N, j.K, &v, &splits, &rows);
      *det_floats += (int64_t)splits * j.N * j.K + (int64_t)splits * j.N;
    }
  });
}

int64_t dw_workspace_floats(const Layout& L, int64_t M, bool with_color) {
  int64_t det, staged;
  dw_sizes(L, M, with_color, &det, &staged);
  if (!(L.variant & RNB_VARIANT_DETERMINISTIC)) return staged;
  return staged + det + (is_bf16(L) ? bf16_dw_floats(L, M, with_color) : 0);
}

// the ordered-reduction part of pb.dw_part for a backward of these parts (the one-workgroup kernel's slabs follow it)
static int64_t dw_det_floats(const Layout& L, const PointBufs& pb, const BwdParts& parts) {
  int64_t det, staged;
  dw_sizes(L, pb.M, parts.albedo || parts.feat, &det, &staged);
  return pb.dw_part_floats - staged;
}

int dw_zero_partials(const Layout& L, const PointBufs& pb, const BwdParts& parts, hipStream_t s) {
  if (pb.dw_part == nullptr) RNB_FAIL(RNB_E_WORKSPACE, "no weight-gradient slab workspace was carved");
  const int64_t det_floats = dw_det_floats(L, pb, parts);
  if ((L.variant & RNB_VARIANT_DETERMINISTIC) && det_floats > 0)
    RNB_CHECK_HIP(hipMemsetAsync(pb.dw_part, 0, (size_t)det_floats * sizeof(float), s));
  return RNB_OK;
}

// Collects the dW jobs of one backward and launches them as (at most) three grouped GEMMs, one per kernel variant
// (K-tile 128 exact / K-tile 64 exact / K-tile 64 guarded), and the one-workgroup-per-gradient kernel.
struct DwBatch {
  DwGroup grp[4];     // [0] K % 128 == 0, [1] K % 64 == 0, [2] anything (guarded), [3] 256 x 256 (LDS-DMA staged)
  double flops[4];
  const Layout& L;
  int64_t M;
  hipStream_t s;
  bool lds_path;      // RNB_VARIANT_DW_LDS: staged-through-LDS kernels (A/B switch)
  bool x3;            // RNB_VARIANT_X3: 256 x 256 jobs through gemm_dw_x3_kernel (same split plan and slabs)
  bool h2;            // RNB_VARIANT_X2H: ... as three fp16 terms, the adjoint operands scaled by their recorded maxima
  float* part;        // RNB_VARIANT_DETERMINISTIC: bump allocator over the zeroed partial-slab workspace (or nullptr)
  int64_t part_left;
  float* slab;        // slabs of the staged 256 x 256 kernel (always; the tail of the same workspace)
  int64_t slab_left;
  float* const slab_base;         // the slab workspace as handed in: every flushed group starts from it again
  const int64_t slab_floats;
  // reduce-only jobs: slabs that OTHER kernels wrote: summed by the reduction launch that follows the last group of
  // weight-gradient jobs, no launch of their own
  DwJob extra[kMaxDwExtra];
  int nextra = 0;
  int add_reduce_only(float* dW, int lddw, float* db, float* part, float* partb, int N, int K, int splits) {
    if (nextra == kMaxDwExtra) RNB_FAIL(RNB_E_INVALID, "too many reduce-only jobs");
    DwJob& j = extra[nextra++];
    memset(&j, 0, sizeof(j));
    j.dW = dW; j.db = db; j.part = part; j.partb = partb;
    j.N = N; j.K = K; j.lddw = lddw; j.splits = splits;
    return RNB_OK;
  }
  DwBatch(const Layout& L_, int64_t M_, float* part_, int64_t part_floats, float* slab_, int64_t slab_floats_,
          hipStream_t s_)
      : L(L_), M(M_), s(s_), lds_path((L_.variant & RNB_VARIANT_DW_LDS) != 0), x3(is_x3(L_)), h2(L_.route.h2), part(part_),
        part_left(part_floats), slab(slab_), slab_left(slab_floats_), slab_base(slab_), slab_floats(slab_floats_) {
    for (int v = 0; v < 4; ++v) { grp[v].njobs = 0; grp[v].M = (int)M_; flops[v] = 0.0; }
  }
  // the staged kernel: every job of the group is split the same way, decided when the group is complete
  int flush_staged(bool final = false) {
    DwGroup& g = grp[3];
    if (g.njobs == 0 && !(final && nextra > 0)) return RNB_OK;
    int total_pairs = 0;   // (work units: x3_job_units)
    for (int q = 0; q < g.njobs; ++q) total_pairs += x3_job_units(g.job[q].npairs, g.job[q].K);
    for (int a = 0, b = g.njobs - 1; a < b; ++a, --b) {   // most recently produced operands first (see flush)
      const DwJob t = g.job[a];
      g.job[a] = g.job[b];
      g.job[b] = t;
    }
    int end = 0;
    int64_t one_each = 0;   // floats of ONE split of every job not yet placed
    for (int q = 0; q < g.njobs; ++q) one_each += (int64_t)g.job[q].N * g.job[q].K + g.job[q].N;
    for (int q = 0; q < g.njobs; ++q) {
      DwJob& j = g.job[q];
      int splits, rows;
      dw_staged_plan(M, x3_job_units(j.npairs, j.K), total_pairs, &splits, &rows);
      {   // never more slabs than the workspace holds (a group smaller than the one the workspace was sized for)
        const int64_t per_split = (int64_t)j.N * j.K + j.N;
        one_each -= per_split;
        int64_t room = slab != nullptr ? slab_left / per_split / (g.njobs - q) : 0;
        // The equal share above counts every remaining job at THIS job's slab size.  With 32 or 64 points every job has one
        // split and the workspace (dw_sizes) holds exactly one slab of each: a 256-column job followed by 64-column ones
        // then computed a share of zero and the backward was refused.  What is left after one split of every later job
        // is this job's to take.
        if (room < 1 && slab != nullptr) room = (slab_left - one_each) / per_split;
        if (room < 1) RNB_FAIL(RNB_E_WORKSPACE, "weight-gradient slab workspace exhausted");
        if (splits > room) {
          splits = (int)room;
          int64_t r = (M + splits - 1) / splits;
          r = (r + kStChunk - 1) / kStChunk * kStChunk;
          rows = (int)r;
          splits = (int)((M + rows - 1) / rows);
        }
      }
      j.splits = splits;
      j.rows_per_split = rows;
      end += splits;
      j.block_end = end;
      const int64_t need = (int64_t)splits * j.N * j.K + (int64_t)splits * j.N;
      if (slab == nullptr || need > slab_left) RNB_FAIL(RNB_E_WORKSPACE, "weight-gradient slab workspace exhausted");
      j.part = slab;
      j.partb = slab + (int64_t)splits * j.N * j.K;
      slab += need;
      slab_left -= need;
    }
    if (end > 0) {   // (two scopes: the class time of the weight-gradient kernel is then its own launch duration, as a kernel trace shows it)
      ProfScope prof(flops[3], s, "dW(x3: 256x256 + narrow jobs)");
      if (x3 && h2) hipLaunchKernelGGL((gemm_dw_x3_kernel<0, 2>), dim3((unsigned)end), dim3(512), 0, s, g);
      else if (x3) hipLaunchKernelGGL((gemm_dw_x3_kernel<0, 3>), dim3((unsigned)end), dim3(512), 0, s, g);
      else hipLaunchKernelGGL(gemm_dw_staged_kernel<0>, dim3((unsigned)end), dim3(1024), 0, s, g);
    }
    RNB_CHECK_LAUNCH();
    int nred = g.njobs;
    if (final) {   // the reduce-only jobs ride behind the real ones (no blocks of the kernel above: block_end stays `end`)
      for (int q = 0; q < nextra; ++q) {
        g.job[nred] = extra[q];
        g.job[nred].block_end = end;
        ++nred;
      }
      nextra = 0;
    }
    {
      ProfScope prof(0.0, s, "dW(slab reduce)");
      hipLaunchKernelGGL(dw_reduce_kernel<0>, dim3(256, nred), dim3(256), 0, s, g);
    }
    g.njobs = 0;
    flops[3] = 0.0;
    // the reduction above has read every slab of this group and the next group's kernels follow it on the same
    // stream: the workspace (sized for ONE group of kMaxDwJobs, dw_sizes) is free again.  Without this a model
    // with more 256-wide gradient jobs than one group holds ran out of slabs on its second group.
    slab = slab_base;
    slab_left = slab_floats;
    RNB_CHECK_LAUNCH();
    return RNB_OK;
  }
  int flush(int v) {
    DwGroup& g = grp[v];
    if (g.njobs == 0) return RNB_OK;
    // Jobs are added in the order the backward produces their operands (layer nh-1 first); launch them
    // most-recent-first so that the operands written last (zb_0, zb_1, ...) are still in the memory-side
    // cache when their job runs.
    for (int a = 0, b = g.njobs - 1; a < b; ++a, --b) {
      const DwJob t = g.job[a];
      g.job[a] = g.job[b];
      g.job[b] = t;
    }
    {
      int end = 0;   // recompute the prefix sums of the block counts for the new order
      for (int q = 0; q < g.njobs; ++q) {
        DwJob& j = g.job[q];
        const int kt = v == 0 ? 128 : 64;
        const int tiles = ((j.N + 127) / 128) * ((j.K + kt - 1) / kt);
        end += (tiles * j.splits + 7) / 8 * 8;
        j.block_end = end;
      }
    }
    const dim3 grid((unsigned)g.job[g.njobs - 1].block_end);
    {
      ProfScope prof(flops[v], s, "dW(other)");
      if (v == 0 && !lds_path) hipLaunchKernelGGL((gemm_dw_direct_kernel<128, 3>), grid, dim3(256), 0, s, g);
      else if (v == 1 && !lds_path) hipLaunchKernelGGL((gemm_dw_direct_kernel<64, 3>), grid, dim3(256), 0, s, g);
      else if (v == 0) hipLaunchKernelGGL((gemm_dw_kernel<false, 128>), grid, dim3(256), 0, s, g);
      else if (v == 1) hipLaunchKernelGGL((gemm_dw_kernel<false, 64>), grid, dim3(256), 0, s, g);
      else hipLaunchKernelGGL((gemm_dw_kernel<true, 64>), grid, dim3(256), 0, s, g);
      if (part != nullptr) {   // ordered reduction of the partial slabs
        RNB_CHECK_LAUNCH();
        hipLaunchKernelGGL(dw_reduce_kernel<0>, dim3(256, g.njobs), dim3(256), 0, s, g);
      }
    }
    g.njobs = 0;
    flops[v] = 0.0;
    RNB_CHECK_LAUNCH();
    return RNB_OK;
  }
  int add(DwPair p1, DwPair p2, int npairs, int N, int K, float* dW, int lddw, float* db, int bias_pair, double fl) {
    int v, splits, rows;
    dw_plan(M, N, K, &v, &splits, &rows);
    if (dw_one_wg(L, M, N, K)) {
      int rc = RNB_OK;
      x3_for_each_range(K, [&](int c0, int width) {
        if (rc != RNB_OK) return;
        if (grp[3].njobs == kMaxDwJobs) rc = flush_staged();
        if (rc != RNB_OK) return;
        DwJob& j = grp[3].job[grp[3].njobs++];
        j.p1 = p1; j.p2 = p2;
        j.p1.Y += c0; j.p2.Y += c0;              // column range of the Y operands (their leading dimension stays)
        j.dW = dW + c0;
        j.db = c0 == 0 ? db : nullptr;            // the bias sums (columns of X) belong to the first range
        j.part = nullptr; j.partb = nullptr;
        j.npairs = npairs; j.N = N; j.K = width; j.lddw = lddw; j.bias_pair = bias_pair;
        j.splits = 0; j.rows_per_split = 0; j.block_end = 0;
      });
      RNB_TRY(rc);
      flops[3] += fl;
      return RNB_OK;
    }
    if (grp[v].njobs == kMaxDwJobs) RNB_TRY(flush(v));
    const int kt = v == 0 ? 128 : 64;
    const int tiles = ((N + 127) / 128) * ((K + kt - 1) / kt);
    DwGroup& g = grp[v];
    DwJob& j = g.job[g.njobs];
    j.p1 = p1; j.p2 = p2; j.dW = dW; j.db = db;
    j.part = nullptr;
    j.partb = nullptr;
    if (part != nullptr) {
      const int64_t need = (int64_t)splits * N * lddw + (int64_t)splits * N;
      if (need > part_left) RNB_FAIL(RNB_E_WORKSPACE, "deterministic dW: partial-slab workspace exhausted");
      j.part = part;
      j.partb = part + (int64_t)splits * N * lddw;
      part += need;
      part_left -= need;
    }
    j.npairs = npairs; j.N = N; j.K = K; j.lddw = lddw; j.bias_pair = bias_pair;
    j.splits = splits; j.rows_per_split = rows;
    // jobs start on a multiple of 8 blocks so that (block & 7) is the XCD inside every job
    const int begin = g.njobs ? g.job[g.njobs - 1].block_end : 0;
    j.block_end = begin + (tiles * splits + 7) / 8 * 8;
    ++g.njobs;
    flops[v] += fl;
    return RNB_OK;
  }
  int flush_all() {
    RNB_TRY(flush(1));   // holds the first layer's job: its operands are the most recent
    RNB_TRY(flush_staged(true));
    RNB_TRY(flush(0));
    return flush(2);
  }
};

// Called after every other launch of the backward: no job reads a buffer that a later launch writes.
int dw_backward(const Layout& L, const PointBufs& pb, const BwdParts& parts, int sdfh_slabs, float* packed_grad, hipStream_t s) {
  const bool det = (L.variant & RNB_VARIANT_DETERMINISTIC) != 0;
  const int64_t det_floats = dw_det_floats(L, pb, parts);
  DwBatch dw(L, pb.M, det ? pb.dw_part : nullptr, det ? det_floats : 0, pb.dw_part + det_floats,
             pb.dw_part_floats - det_floats, s);
  int rc = RNB_OK;
  dw_list(L, pb, parts, sdfh_slabs, [&](const DwListed& j) {
    if (rc != RNB_OK) return;
    float* dW = packed_grad + j.w_off;
    float* db = packed_grad + j.b_off;
    if (j.splits > 0) rc = dw.add_reduce_only(dW, j.K, db, j.part, j.partb, j.N, j.K, j.splits);
    else rc = dw.add(j.p1, j.p2, j.npairs, j.N, j.K, dW, j.K, db, j.bias_pair, j.flops);
  });
  RNB_TRY(rc);
  return dw.flush_all();
}

}  // namespace rnb
