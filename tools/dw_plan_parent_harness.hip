// The weight-gradient launches of commit 8adcc79 (the parent of the planner in csrc/dw_plan.h), recorded without a GPU.
// TEST INFRASTRUCTURE ONLY.  This file applies to THAT commit: it includes its csrc/dw.hip unmodified, with the launch
// macro replaced by a function that writes down the DwGroup it is given, runs dw_backward on the CPU over a PointBufs
// whose buffers are addresses only, and prints every launch.  tools/gen_dw_plan_golden.py checks that commit's csrc out
// into a scratch directory, builds this file against it and writes tests/golden/dw_plan_parent.json.
//
//   hipcc --cuda-host-only -std=c++17 -I <csrc of 8adcc79> tools/dw_plan_parent_harness.hip <that csrc>/layout.hip -o harness
#include <hip/hip_runtime.h>

#include "rnb_internal.h"
#include "dw_plan_cases.h"

namespace rnb {
static DumpCase* g_case = nullptr;
static const PointBufs* g_pb = nullptr;
template <class Group>
static void record_launch(const char* kernel, dim3 grid, dim3 block, const Group& g) {
  auto grad = [](const float* p) { return p == nullptr ? -1LL : (long long)(p - (const float*)kFakeGrad); };
  auto slab = [](const float* p) { return p == nullptr ? -1LL : (long long)(p - g_pb->dw_part); };
  std::vector<DumpJob> jobs;
  for (int q = 0; q < g.njobs; ++q) {
    const auto& j = g.job[q];
    jobs.push_back(DumpJob{{grad(j.dW), grad(j.db), j.N, j.K, j.lddw, j.npairs, j.bias_pair, j.splits, j.rows_per_split,
                            j.block_end, slab(j.part), slab(j.partb)}});
  }
  if (std::string(kernel) != "dw_reduce_kernel<0>") {
    DumpLaunch l;
    l.kernel = kernel;
    if (l.kernel[0] == '(') l.kernel = l.kernel.substr(1, l.kernel.size() - 2);
    l.grid = (int)grid.x; l.block = (int)block.x; l.M = g.M;
    l.jobs = jobs;
    g_case->launches.push_back(l);
    return;
  }
  // the reduction of the launch before it (the same group), or of reduce-only jobs alone
  if (g.njobs == 0) {
    DumpLaunch l;
    l.kernel = "none";
    l.M = g.M;
    g_case->launches.push_back(l);
  }
  DumpLaunch& l = g_case->launches.back();
  bool same = l.nreduce == 0 && l.jobs.size() == jobs.size() && grid.x == 256 && block.x == 256;
  for (size_t q = 0; same && q < jobs.size(); ++q) same = memcmp(&l.jobs[q], &jobs[q], sizeof(DumpJob)) == 0;
  if (!same) { fprintf(stderr, "a slab reduction that does not follow its own group\n"); exit(2); }
  l.nreduce = (int)grid.y;
  for (int q = g.njobs; q < (int)grid.y; ++q) {
    const auto& j = g.job[q];
    const bool sdfh = j.part == g_pb->sdfh_part;
    if (!sdfh && j.part != g_pb->col_part) { fprintf(stderr, "a reduce-only job of unknown slabs\n"); exit(2); }
    l.extra.push_back(DumpExtra{{grad(j.dW), grad(j.db), j.N, j.K, j.lddw, j.splits, j.block_end, sdfh, (long long)(j.partb - j.part)}});
  }
}
}  // namespace rnb

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, group) ::rnb::record_launch(#kernel, grid, block, group)
#define hipGetLastError() hipSuccess   // (no device here: the launches above cannot fail)
#include "dw.hip"

int main() {
  using namespace rnb;
  char tag[8];
  while (scanf("%7s", tag) == 1) {
    CaseIn in;
    if (tag[0] != 'D' || !read_case(&in)) { fprintf(stderr, "bad case line\n"); return 2; }
    DumpCase out;
    Layout L;
    PointBufs pb;
    if (setup_case(in, &L, &pb, &out)) {
      g_case = &out;
      g_pb = &pb;
      out.dw_part_floats = pb.dw_part_floats;
      out.slab_off = dw_det_floats(L, pb, in.parts);
      out.rc = dw_backward(L, pb, in.parts, in.slabs, (float*)kFakeGrad, nullptr);
      if (out.rc != RNB_OK) out.error = last_error();
    }
    print_case(out);
  }
  return 0;
}
