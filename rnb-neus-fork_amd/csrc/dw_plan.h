// The weight-gradient ("dW") launches of one backward as DATA: dw_make_plan turns the job shapes of dw_list (dw.hip) into
// the launches (kernel, grid, per job its column range, point split and slab offsets in PointBufs::dw_part) and the two
// workspace totals.  Sizing (dw_workspace_floats) and launch (dw_backward) read it; tools/dw_plan_dump.hip prints it and
// tests/test_dw_plan_host.py holds it to recorded plans.  Plain C++17, no HIP include, no heap: it runs in every backward.
#pragma once
#include <stdint.h>

#include "../../include/rnbneus.h"

namespace rnb {

constexpr int BK = 32;            // points per main-loop step of the GEMM kernels (gemm.hip.h): a split-K split is a multiple
constexpr int kStChunk = 32;      // points per chunk of the one-workgroup kernels (dw.hip.h): their splits are multiples
constexpr int kMaxDwJobs = 12;    // jobs of one launch (DwGroup)
constexpr int kMaxDwExtra = 2;    // reduce-only jobs (slabs written by other kernels) that ride in the reduction launch
constexpr int kMaxDwListed = 40;  // jobs of one backward (dw_list: at most 2 x 15 layers + 3)
constexpr int kMaxDwLaunches = 16;
constexpr int64_t kDwUnbounded = INT64_MAX / 4;   // slab room of a sizing plan

// split-K plan of one dW job: kernel variant v ([0] K % 128 == 0, [1] K % 64 == 0, [2] anything: guarded), number of
// point splits and points per split.
inline void dw_plan(int64_t M, int N, int K, int* v_out, int* splits_out, int* rows_out) {
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
// blocks of a split-K job: jobs start on a multiple of 8 blocks so that (block & 7) is the XCD inside every job
inline int dw_job_blocks(int v, int N, int K, int splits) {
  const int kt = v == 0 ? 128 : 64;
  return (((N + 127) / 128) * ((K + kt - 1) / kt) * splits + 7) / 8 * 8;
}

// Point split of the staged 256 x 256 kernel: one workgroup per (job, split) and ONE round of workgroups (<= 256, one per
// CU), each job's share of them proportional to its work (operand pairs), so every CU multiplies for the whole launch.
// Partial gradients leave through plain stores into slabs that dw_reduce_kernel sums in split order: an fp32 atomic tail
// of 256 KB per workgroup would cost ~50 us per round at the chip's ~1.3 TB/s atomic rate, with nothing to hide under.
// (Restated in Python, with dw_make_plan's room clamp, by tests/point_matrix.py: a change here changes that table's rows.)
inline void dw_staged_plan(int64_t M, int npairs, int total_pairs, int* splits_out, int* rows_out) {
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
inline bool x3_job_shape(bool x3, int N, int K) { return N == 256 && (K == 256 || (x3 && K % 64 == 0 && K >= 64 && K <= 1024)); }
inline int x3_job_units(int npairs, int width) { return npairs * (width >= 256 ? 2 : 1); }
template <class F>
inline void x3_for_each_range(int K, F f) {   // f(first column, width): 256-wide ranges, then 64-wide ones
  int c = 0;
  for (; c + 256 <= K; c += 256) f(c, 256);
  for (; c + 64 <= K; c += 64) f(c, 64);
}

struct DwShape { int N, K, npairs; };   // one job of dw_list, in its order; npairs == 0: a reduce-only job
// The routing options, from the variant bits and M (dw.hip dw_routing): x3 arithmetic; x2h operand form; the
// one-workgroup kernel runs (dw_one_wg_runs) and then takes every job of its shape; RNB_VARIANT_DW_LDS;
// RNB_VARIANT_DETERMINISTIC (split-K partials through ordered-reduction slabs instead of fp32 atomics).
struct DwRouting { bool x3, h2, one_wg, lds, det; };
enum DwKernel {
  DW_K_DIRECT128, DW_K_DIRECT64,          // gemm_dw_direct_kernel<128 / 64, 3>: K % 128 == 0 / K % 64 == 0
  DW_K_LDS128, DW_K_LDS64, DW_K_GUARDED,  // gemm_dw_kernel<false, 128 / 64> (RNB_VARIANT_DW_LDS), <true, 64>: anything
  DW_K_X3_H2, DW_K_X3, DW_K_STAGED,       // one workgroup per (job, split): gemm_dw_x3_kernel<0, 2 / 3>, gemm_dw_staged_kernel<0>
  DW_K_NONE,                              // no kernel: only reduce-only jobs are left for the slab reduction
  DW_K_REDUCE                             // (dw_reduce_kernel<0>, which follows a launch with nreduce > 0: never a launch's own)
};
struct DwPlanJob {
  int src, col0;           // job of the list and first column of its range [col0, col0 + K)
  int N, K, npairs, splits, rows_per_split, block_end;
  int64_t part, partb;     // partial slabs [splits][N][K] and [splits][N]: float offsets from dw_part, or -1 (fp32 atomics)
};
struct DwLaunch {
  int kernel, grid, block, njobs;
  DwPlanJob job[kMaxDwJobs];        // in launch order
  int nreduce;                      // > 0: dw_reduce_kernel<0> follows over this many jobs: the launch's own, then `extra`
  int extra[kMaxDwExtra];           // reduce-only jobs of the list that ride in that reduction
};
struct DwPlan {
  int rc;                           // RNB_OK, or why there is no plan (RNB_E_WORKSPACE: the jobs do not fit the rooms)
  const char* error;
  int nlaunches;
  DwLaunch launch[kMaxDwLaunches];  // in launch order
  // The two parts of PointBufs::dw_part these jobs are SIZED with: ordered-reduction slabs of the jobs the split-K kernels
  // take, and slabs for every job of the one-workgroup kernel's shape, whether the variant routes it there or not, split as
  // ONE group.  (A backward with fewer operand pairs per job, or more jobs than one group, splits finer and is held to
  // the room below.)
  int64_t det_floats, slab_floats;
};

// The plan of the jobs `jobs` over M points.  det_room: floats of the ordered-reduction part of dw_part (from offset 0);
// slab_base, slab_room: offset and floats of the one-workgroup kernel's part; kDwUnbounded rooms give the sizing plan.
inline void dw_make_plan(const DwShape* jobs, int njobs, int64_t M, const DwRouting& r, int64_t det_room, int64_t slab_base,
                         int64_t slab_room, DwPlan* P) {
  P->rc = RNB_OK, P->error = "";
  P->nlaunches = 0, P->det_floats = P->slab_floats = 0;
  auto fail = [&](int rc, const char* msg) { if (P->rc == RNB_OK) { P->rc = rc; P->error = msg; } };
  auto one_wg = [&](const DwShape& j) { return r.one_wg && x3_job_shape(r.x3, j.N, j.K); };   // the routing rule
  // ---- the totals (reduce-only jobs are other kernels' slabs, carved with their producers: no room of their own) ----
  int total_units = 0;
  for (int i = 0; i < njobs; ++i)
    if (jobs[i].npairs > 0 && x3_job_shape(r.x3, jobs[i].N, jobs[i].K))
      x3_for_each_range(jobs[i].K, [&](int, int width) { total_units += x3_job_units(jobs[i].npairs, width); });
  for (int i = 0; i < njobs; ++i) {
    const DwShape& j = jobs[i];
    int v, splits, rows;
    if (j.npairs > 0 && x3_job_shape(r.x3, j.N, j.K))
      x3_for_each_range(j.K, [&](int, int width) {
        dw_staged_plan(M, x3_job_units(j.npairs, width), total_units, &splits, &rows);
        P->slab_floats += (int64_t)splits * j.N * width + (int64_t)splits * j.N;
      });
    // (jobs of the one-workgroup kernel leave through its own slabs, whatever the variant: no ordered-reduction slabs —
    // and no 200 MB memset per step — for them)
    if (j.npairs > 0 && !one_wg(j)) {
      dw_plan(M, j.N, j.K, &v, &splits, &rows);
      P->det_floats += (int64_t)splits * j.N * j.K + (int64_t)splits * j.N;
    }
  }
  // ---- the launches: a group per kernel class ([0] K-tile 128, [1] K-tile 64, [2] guarded, [3] one-workgroup) ----
  DwLaunch grp[4];
  for (int v = 0; v < 4; ++v) grp[v].njobs = 0;
  int extra[kMaxDwExtra], nextra = 0;
  int64_t det_next = 0;
  // Jobs are listed in the order the backward produces their operands (layer nh-1 first) and launched most-recent-first,
  // so that the operands written last (zb_0, zb_1, ...) are still in the memory-side cache when their job runs.
  auto emit = [&](DwLaunch& g) {
    if (P->nlaunches == kMaxDwLaunches) return fail(RNB_E_INVALID, "too many weight-gradient launches");   // (nothing is added after a failure)
    DwLaunch& out = P->launch[P->nlaunches++];
    out = g;
    for (int q = 0; q < g.njobs; ++q) out.job[q] = g.job[g.njobs - 1 - q];
    g.njobs = 0;
  };
  auto flush = [&](int v) {
    DwLaunch& g = grp[v];
    if (g.njobs == 0) return;
    int end = 0;   // prefix sums of the block counts, in launch order
    for (int q = g.njobs - 1; q >= 0; --q) g.job[q].block_end = end += dw_job_blocks(v, g.job[q].N, g.job[q].K, g.job[q].splits);
    g.kernel = v == 2 ? DW_K_GUARDED : (r.lds ? DW_K_LDS128 : DW_K_DIRECT128) + v;
    g.grid = end;
    g.block = 256;
    g.nreduce = r.det ? g.njobs : 0;   // ordered reduction of the partial slabs
    emit(g);
  };
  // the one-workgroup kernel: every job of the group is split the same way, decided when the group is complete.  Its slab
  // reduction reads every slab of the group and the next group's kernels follow it on the same stream: each group has
  // the whole slab room.  final: the reduce-only jobs ride behind the real ones (no blocks of the kernel: block_end = grid)
  auto flush_one_wg = [&](bool final) {
    DwLaunch& g = grp[3];
    if (g.njobs == 0 && !(final && nextra > 0)) return;
    int total_pairs = 0, end = 0;   // (work units: x3_job_units)
    int64_t one_each = 0, used = 0;   // floats of ONE split of every job not yet placed; floats placed
    for (int q = 0; q < g.njobs; ++q) {
      total_pairs += x3_job_units(g.job[q].npairs, g.job[q].K);
      one_each += (int64_t)g.job[q].N * g.job[q].K + g.job[q].N;
    }
    for (int q = g.njobs - 1; q >= 0; --q) {   // launch order: q + 1 jobs are not yet placed
      DwPlanJob& j = g.job[q];
      int splits, rows;
      dw_staged_plan(M, x3_job_units(j.npairs, j.K), total_pairs, &splits, &rows);
      // never more slabs than the room holds (a group smaller than the one the workspace was sized for)
      const int64_t per_split = (int64_t)j.N * j.K + j.N, slab_left = slab_room - used;
      one_each -= per_split;
      int64_t room = slab_left / per_split / (q + 1);
      // The equal share above counts every remaining job at THIS job's slab size.  With 32 or 64 points every job has one
      // split and the workspace holds exactly one slab of each: a 256-column job followed by 64-column ones then
      // computed a share of zero and the backward was refused.  What is left after one split of every later job is this
      // job's to take.
      if (room < 1) room = (slab_left - one_each) / per_split;
      if (room < 1) return fail(RNB_E_WORKSPACE, "weight-gradient slab workspace exhausted");
      if (splits > room) {
        splits = (int)room;
        int64_t rw = (M + splits - 1) / splits;
        rows = (int)((rw + kStChunk - 1) / kStChunk * kStChunk);
        splits = (int)((M + rows - 1) / rows);
      }
      j.splits = splits;
      j.rows_per_split = rows;
      j.block_end = end += splits;
      j.part = slab_base + used;
      j.partb = j.part + (int64_t)splits * j.N * j.K;
      used += splits * per_split;
    }
    g.kernel = end == 0 ? DW_K_NONE : !r.x3 ? DW_K_STAGED : r.h2 ? DW_K_X3_H2 : DW_K_X3;
    g.grid = end;
    g.block = r.x3 ? 512 : 1024;
    g.nreduce = g.njobs + (final ? nextra : 0);
    for (int q = 0; q < nextra; ++q) g.extra[q] = extra[q];
    emit(g);
  };
  for (int i = 0; i < njobs && P->rc == RNB_OK; ++i) {
    const DwShape& j = jobs[i];
    if (j.npairs == 0) {
      if (nextra == kMaxDwExtra) return fail(RNB_E_INVALID, "too many reduce-only jobs");
      extra[nextra++] = i;
    } else if (one_wg(j)) {
      x3_for_each_range(j.K, [&](int c0, int width) {
        if (grp[3].njobs == kMaxDwJobs) flush_one_wg(false);
        if (P->rc != RNB_OK) return;
        grp[3].job[grp[3].njobs++] = DwPlanJob{i, c0, j.N, width, j.npairs, 0, 0, 0, -1, -1};
      });
    } else {
      int v, splits, rows;
      dw_plan(M, j.N, j.K, &v, &splits, &rows);
      if (grp[v].njobs == kMaxDwJobs) flush(v);
      if (P->rc != RNB_OK) return;
      DwPlanJob& p = grp[v].job[grp[v].njobs++] = DwPlanJob{i, 0, j.N, j.K, j.npairs, splits, rows, 0, -1, -1};
      if (r.det) {
        const int64_t need = (int64_t)splits * j.N * j.K + (int64_t)splits * j.N;
        if (need > det_room - det_next) return fail(RNB_E_WORKSPACE, "deterministic dW: partial-slab workspace exhausted");
        p.part = det_next;
        p.partb = det_next + (int64_t)splits * j.N * j.K;
        det_next += need;
      }
    }
  }
  if (P->rc != RNB_OK) return;
  flush(1);   // holds the first layer's job: its operands are the most recent
  flush_one_wg(true);
  flush(0);
  flush(2);
}

}  // namespace rnb
