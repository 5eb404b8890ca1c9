// Prints the weight-gradient launch plan (csrc/dw_plan.h) as JSON, one line per case read from stdin.  No GPU: host only.
//   D <descriptor> M <BwdParts> <carve mode> sdfh_slabs   the plan dw_backward launches (line format: dw_plan_cases.h)
//   J M x3 h2 one_wg lds det det_room slab_base slab_room n {N K npairs} x n
//                                                         dw_make_plan of bare job shapes (a negative room: unbounded)
//   B <descriptor> M with_color                           the grouped launch of the bf16 route (csrc/bf16_dw_plan.h): per job
//                                                         [kind, layer, K, lddw, npairs, bias_pair, ycol0, with_bias, slab_off]
// tests/test_dw_plan_host.py and tests/test_bf16_point_matrix_host.py build and run it.  Not part of the library:
//   hipcc --cuda-host-only -std=c++17 -I rnb-neus-fork_amd/csrc tools/dw_plan_dump.hip rnb-neus-fork_amd/csrc/layout.hip -o dw_plan_dump
#include <hip/hip_runtime.h>
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) ((void)0)   // nothing here launches: a host-only build has no device code to refer to
#include "dw.hip"   // (for dw_list and dw_plan_parts)
#include "dw_plan_cases.h"

namespace rnb {
static const char* const kKernelNames[] = {"gemm_dw_direct_kernel<128, 3>", "gemm_dw_direct_kernel<64, 3>", "gemm_dw_kernel<false, 128>",
                                           "gemm_dw_kernel<false, 64>", "gemm_dw_kernel<true, 64>", "gemm_dw_x3_kernel<0, 2>",
                                           "gemm_dw_x3_kernel<0, 3>", "gemm_dw_staged_kernel<0>", "none", "dw_reduce_kernel<0>"};

// job == nullptr: bare shapes, whose gradient offsets are the job's index in the list and its first column
static void dump_plan(const DwPlan& P, const DwListed* job, const PointBufs* pb, int64_t M, DumpCase* out) {
  out->rc = P.rc;
  out->error = P.error;
  for (int i = 0; i < P.nlaunches && P.rc == RNB_OK; ++i) {
    const DwLaunch& pl = P.launch[i];
    DumpLaunch l;
    l.kernel = kKernelNames[pl.kernel];
    l.grid = pl.grid;
    l.block = pl.grid > 0 ? pl.block : 0;
    l.M = (int)M;
    l.nreduce = pl.nreduce;
    for (int q = 0; q < pl.njobs; ++q) {
      const DwPlanJob& p = pl.job[q];
      const long long dW = job ? job[p.src].w_off + p.col0 : p.src, db = job ? (p.col0 == 0 ? job[p.src].b_off : -1) : p.col0;
      const int lddw = job ? job[p.src].K : p.K, bias_pair = job ? job[p.src].bias_pair : 0;
      l.jobs.push_back(DumpJob{{dW, db, p.N, p.K, lddw, p.npairs, bias_pair, p.splits, p.rows_per_split, p.block_end, p.part, p.partb}});
    }
    for (int q = pl.njobs; q < pl.nreduce; ++q) {
      const int src = pl.extra[q - pl.njobs];
      if (job == nullptr) { l.extra.push_back(DumpExtra{{src, -1, 0, 0, 0, 0, pl.grid, 0, 0}}); continue; }
      const DwListed& j = job[src];
      l.extra.push_back(DumpExtra{{j.w_off, j.b_off, j.N, j.K, j.K, j.splits, pl.grid, j.part == pb->sdfh_part, (long long)(j.partb - j.part)}});
    }
    out->launches.push_back(l);
  }
}
}  // namespace rnb

// a "B" line: the bf16 route's plan of (descriptor, M, with_color)
static bool dump_bf16_case() {
  using namespace rnb;
  rnb_model_desc desc;
  long long M;
  int with_color;
  if (!read_desc(&desc) || scanf("%lld %d", &M, &with_color) != 2) return false;
  Layout L;
  const int rc = make_layout(&desc, &L);
  if (rc != RNB_OK) {
    printf("{\"refused\":%d,\"error\":\"%s\"}\n", rc, last_error());
    return true;
  }
  BfDwShape shape[kBfDwListed];
  const int n = bf16_dw_shapes(bf16_dw_net(L), with_color != 0, shape);
  const BfDwSplit S = bf16_dw_split(shape, n, M);
  printf("{\"njobs\":%d,\"want\":%d,\"rows\":%lld,\"splits\":%d,\"total\":%lld,\"sdf_route\":%d,\"color_route\":%d,\"jobs\":[", n, S.want,
         (long long)S.rows_per_split, S.splits, (long long)S.total, (int)L.route.sdf, (int)L.route.color);
  for (int q = 0; q < n; ++q) {
    const BfDwShape& j = shape[q];
    printf("%s[%d,%d,%d,%d,%d,%d,%d,%d,%lld]", q ? "," : "", j.kind, j.layer, j.K, j.lddw, j.npairs, j.bias_pair, j.ycol0, (int)j.with_bias,
           q < kMaxBfDwJobs ? (long long)S.slab_off[q] : -1LL);
  }
  printf("]}\n");
  return true;
}

int main() {
  using namespace rnb;
  char tag[8];
  while (scanf("%7s", tag) == 1) {
    if (tag[0] == 'B') {
      if (!dump_bf16_case()) { fprintf(stderr, "bad bf16 line\n"); return 2; }
      continue;
    }
    DumpCase out;
    DwPlan P;
    if (tag[0] == 'D') {
      CaseIn in;
      if (!read_case(&in)) { fprintf(stderr, "bad case line\n"); return 2; }
      Layout L;
      PointBufs pb;
      DwListed job[kMaxDwListed];
      if (setup_case(in, &L, &pb, &out)) {
        out.dw_part_floats = pb.dw_part_floats;
        out.slab_off = pb.dw_slab_off;
        dw_plan_parts(L, pb, in.parts, in.slabs, false, job, &P);
        dump_plan(P, job, &pb, in.M, &out);
      }
    } else {
      long long M, det_room, slab_base, slab_room;
      int b[5], n;
      if (scanf("%lld %d %d %d %d %d %lld %lld %lld %d", &M, &b[0], &b[1], &b[2], &b[3], &b[4], &det_room, &slab_base, &slab_room, &n) != 10 ||
          n < 0 || n > kMaxDwListed) { fprintf(stderr, "bad job line\n"); return 2; }
      DwShape shape[kMaxDwListed];
      for (int i = 0; i < n; ++i)
        if (scanf("%d %d %d", &shape[i].N, &shape[i].K, &shape[i].npairs) != 3) { fprintf(stderr, "bad job line\n"); return 2; }
      dw_make_plan(shape, n, M, DwRouting{b[0] != 0, b[1] != 0, b[2] != 0, b[3] != 0, b[4] != 0}, det_room < 0 ? kDwUnbounded : det_room,
                   slab_base, slab_room < 0 ? kDwUnbounded : slab_room, &P);
      out.dw_part_floats = P.det_floats;   // (the two totals of the plan)
      out.slab_off = P.slab_floats;
      dump_plan(P, nullptr, nullptr, M, &out);
    }
    print_case(out);
  }
  return 0;
}
