// The grouped weight-gradient launch of the bf16 route (bf16_dw.hip bf_dw_kernel) as DATA: which jobs one backward lists, in
// launch order, and how the points are split over workgroups.  bf16_dw.hip attaches operands and targets to these shapes and
// launches them; sizing (bf16_dw_floats) reads the same plan; tools/dw_plan_dump.hip prints it and
// tests/test_bf16_point_matrix_host.py holds the restatement of tests/bf16_point_matrix.py to it.  Plain C++17, no HIP
// include, no heap (like dw_plan.h): it runs in every backward.
#pragma once
#include <stdint.h>

#include "../../include/rnbneus.h"

namespace rnb {

constexpr int kMaxBfDwJobs = 16;    // jobs of one launch (BfDwGroup)
constexpr int kBfDwListed = 2 * RNB_MAX_LIN + 2;   // jobs one backward can list: hidden layers, feature head, albedo layers (+ 1)
constexpr int kBfDwRows = 256;      // every job's dW has 256 rows (the X operand's columns)
constexpr int kBfDwSplitRows = 64;  // a workgroup's point range is a multiple of this (two 32-point chunks of the LDS ring)
constexpr int kBfDwWant = 512;      // workgroups wanted per launch: njobs x splits >= ~2 per CU

// What the plan reads of the two networks (Layout: hid[l].Kp, feat.Kp, col[l].Kp, Cinp, route.color == COLOR_BF16)
struct BfDwNet {
  int nh, hid_Kp[RNB_MAX_LIN];
  int feat_Kp;
  bool bf16_color;
  int nc, col_Kp[RNB_MAX_LIN], Cinp;
};

// One listed job: dW[256 x K] into columns [ycol0, ycol0 + K) of a [256 x lddw] gradient, summed over npairs operand pairs.
enum BfDwKind { BF_DW_HIDDEN, BF_DW_FEAT, BF_DW_ALBEDO_HIDDEN, BF_DW_ALBEDO_IN_FEAT, BF_DW_ALBEDO_IN_PE };
struct BfDwShape {
  int kind, layer;     // BfDwKind and the layer of its network (0 for the feature head)
  int K, lddw, npairs, bias_pair, ycol0;
  bool with_bias;
};

// The jobs of one bf16 backward, in launch order: the hidden layers 0 .. nh-1 (pairs gz_l / u_l and zb_l / in_l), the feature
// head (with_color), and on the bf16 albedo route the albedo net's layers nc-1 .. 1 and its layer 0 as two jobs (the 256
// feature columns, the encoding columns).  Returns their number (<= kBfDwListed).
inline int bf16_dw_shapes(const BfDwNet& n, bool with_color, BfDwShape* out) {
  int q = 0;
  for (int l = 0; l < n.nh; ++l) out[q++] = BfDwShape{BF_DW_HIDDEN, l, n.hid_Kp[l], n.hid_Kp[l], 2, 1, 0, true};
  if (!with_color) return q;
  out[q++] = BfDwShape{BF_DW_FEAT, 0, n.feat_Kp, n.feat_Kp, 1, 0, 0, true};
  if (!n.bf16_color) return q;
  for (int l = n.nc - 1; l >= 1; --l) out[q++] = BfDwShape{BF_DW_ALBEDO_HIDDEN, l, n.col_Kp[l], n.col_Kp[l], 1, 0, 0, true};
  // layer 0 reads the Cinp-wide input: its 256 feature columns and its pe columns are two jobs
  out[q++] = BfDwShape{BF_DW_ALBEDO_IN_FEAT, 0, kBfDwRows, n.col_Kp[0], 1, 0, 0, true};
  out[q++] = BfDwShape{BF_DW_ALBEDO_IN_PE, 0, n.Cinp - kBfDwRows, n.col_Kp[0], 1, 0, kBfDwRows, false};
  return q;
}

// How the M points of every job are split, and where each job's ordered-reduction slabs lie (deterministic variant).
struct BfDwSplit {
  int want;                            // workgroups wanted per job
  int64_t rows_per_split;
  int splits;
  int64_t slab_off[kMaxBfDwJobs];      // float offset of job q's [splits][256][lddw] slabs; its [splits][256] bias slabs follow
  int64_t total;                       // floats of all slabs, of every listed job
};
// njobs: the jobs listed (the launch holds the first kMaxBfDwJobs of them; more are refused at the launch)
inline BfDwSplit bf16_dw_split(const BfDwShape* jobs, int njobs, int64_t M) {
  BfDwSplit S{};
  // points per workgroup: enough workgroups to fill the chip, ranges a multiple of 64
  S.want = (kBfDwWant + njobs - 1) / njobs;
  S.rows_per_split = ((M + S.want - 1) / S.want + kBfDwSplitRows - 1) / kBfDwSplitRows * kBfDwSplitRows;
  S.splits = (int)((M + S.rows_per_split - 1) / S.rows_per_split);
  const int64_t slab = (int64_t)S.splits * kBfDwRows;   // floats per column of lddw + 1
  for (int q = 0; q < njobs; ++q) S.total += slab * (jobs[q].lddw + 1);
  for (int q = 1; q < njobs && q < kMaxBfDwJobs; ++q) S.slab_off[q] = S.slab_off[q - 1] + slab * (jobs[q - 1].lddw + 1);
  return S;
}

}  // namespace rnb
