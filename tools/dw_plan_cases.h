// Shared by tools/dw_plan_dump.hip (the planner of this tree) and tools/dw_plan_parent_harness.hip (the launches of the
// commit before the planner existed): one case per input line, one JSON line per case, the same fields in the same order,
// so that tests/test_dw_plan_host.py can compare them text for text.  Host only; include after rnb_internal.h.
//
// A case line:  D <the 19 int fields of rnb_model_desc in order; sdf_scale = 1> M albedo sdf feat normal color_inputs mode slabs
//   (the five BwdParts flags, the PointMode bits the workspace is carved with, sdfh_slabs)
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

namespace rnb {

// ---- what the planning code links against besides layout.hip, answered as the library answers it ----
bool prof_enabled() { return false; }
void prof_begin(double, hipStream_t, const char*) {}
void prof_end(hipStream_t) {}
int64_t bf16_dw_floats(const Layout&, int64_t, bool) { return 0; }   // (the bf16 route plans its own jobs: not in the matrix)
bool fused_supported(const Layout& L) {   // fused.hip
  if (L.Hp != 256 || L.H != 256) return false;
  if (L.Ep > 64 || L.pe > 40) return false;
  if (L.nh < 1) return false;
  for (int l = 0; l < L.nh; ++l)
    if (L.hid[l].Np != 256 || (L.hid[l].Kp != 256 && l != 0)) return false;
  if (L.F > 256 || (L.F > 0 && L.Fp != 256)) return false;
  return true;
}
bool color_h2_supported(const Layout& L) {   // color_h2.hip
  return is_x2h(L) && !is_bf16(L) && L.F == 256 && L.nc == 2 && L.Hc == 256 && L.Hcp == 256 && L.Cinp - L.F == 64 && L.Co >= 1 &&
         L.Co <= 4 && L.Ep == 64 && 2 * L.pev <= 64 && L.col[0].Kp == L.Cinp && L.col[1].Kp == 256;
}
bool bf16_color_supported(const Layout& L) {   // bf16_color.hip
  if (L.F != 256 || L.Hc != 256 || L.Hcp != 256) return false;
  if (L.Cinp > 320 || L.Cinp % 64 != 0 || L.Cinp - L.F > 64) return false;
  return L.nc >= 1 && L.Co >= 1 && L.Co <= 4;
}
int64_t color_h2_part_floats(const Layout& L, int64_t M) { return (pad_rows(M) / 64) * (int64_t)L.Co * (256 + 1); }

// ---- one case ----
struct DumpJob { long long v[12]; };     // dW, db (float offsets in the packed gradient, -1: none), N, K, lddw, npairs, bias_pair,
                                         // splits, rows_per_split, block_end, part, partb (float offsets in dw_part, -1: atomics)
struct DumpExtra { long long v[9]; };    // dW, db, N, K, lddw, splits, block_end, slab buffer (0 col_part, 1 sdfh_part), partb - part
struct DumpLaunch {
  std::string kernel;                    // as written at the launch, or "none"
  int grid = 0, block = 0, M = 0, nreduce = 0;
  std::vector<DumpJob> jobs;
  std::vector<DumpExtra> extra;
};
struct DumpCase {
  int rc = 0;
  std::string error;
  long long dw_part_floats = 0, slab_off = 0;
  std::vector<DumpLaunch> launches;
};

inline void print_case(const DumpCase& c) {
  if (c.rc != 0) {
    printf("{\"refused\":%d,\"error\":\"%s\"}\n", c.rc, c.error.c_str());
    return;
  }
  printf("{\"floats\":%lld,\"slab_off\":%lld,\"launches\":[", c.dw_part_floats, c.slab_off);
  for (size_t i = 0; i < c.launches.size(); ++i) {
    const DumpLaunch& l = c.launches[i];
    printf("%s{\"kernel\":\"%s\",\"grid\":%d,\"block\":%d,\"M\":%d,\"jobs\":[", i ? "," : "", l.kernel.c_str(), l.grid, l.block, l.M);
    for (size_t q = 0; q < l.jobs.size(); ++q) {
      printf("%s[", q ? "," : "");
      for (int k = 0; k < 12; ++k) printf("%s%lld", k ? "," : "", l.jobs[q].v[k]);
      printf("]");
    }
    printf("],\"nreduce\":%d,\"extra\":[", l.nreduce);
    for (size_t q = 0; q < l.extra.size(); ++q) {
      printf("%s[", q ? "," : "");
      for (int k = 0; k < 9; ++k) printf("%s%lld", k ? "," : "", l.extra[q].v[k]);
      printf("]");
    }
    printf("]}");
  }
  printf("]}\n");
}

struct CaseIn {
  rnb_model_desc desc;
  long long M;
  BwdParts parts;
  int mode, slabs;
};
// the 19 int fields of a descriptor
inline bool read_desc(rnb_model_desc* d) {
  int32_t* f[] = {&d->sdf_d_in, &d->sdf_d_out, &d->sdf_d_hidden, &d->sdf_n_layers, &d->sdf_skip_in,
                  &d->sdf_multires, &d->sdf_weight_norm, &d->col_d_feature, &d->col_d_in, &d->col_d_out,
                  &d->col_d_hidden, &d->col_n_layers, &d->col_multires_view, &d->col_squeeze_out,
                  &d->col_weight_norm, &d->n_samples, &d->n_importance, &d->up_sample_steps, &d->variant};
  d->sdf_scale = 1.f;
  for (int32_t* p : f)
    if (scanf("%d", p) != 1) return false;
  return true;
}
// the rest of a "D" line
inline bool read_case(CaseIn* c) {
  if (!read_desc(&c->desc)) return false;
  int b[5];
  if (scanf("%lld %d %d %d %d %d %d %d", &c->M, &b[0], &b[1], &b[2], &b[3], &b[4], &c->mode, &c->slabs) != 8) return false;
  c->parts = BwdParts{b[0] != 0, b[1] != 0, b[2] != 0, b[3] != 0, b[4] != 0};
  return true;
}

// Layout and carved (buffer-less but addressed) PointBufs of a case, or why the library refuses it before any backward:
// make_layout's own refusals, api.hip's "model has no feature head" for the colour / feature parts of a model without, and
// backward.hip's check_route_buffers for the slabs of reduce-only jobs that the carving mode left out.
constexpr uintptr_t kFakeWorkspace = (uintptr_t)1 << 44, kFakeGrad = (uintptr_t)1 << 45;
inline bool setup_case(const CaseIn& in, Layout* L, PointBufs* pb, DumpCase* out) {
  out->rc = make_layout(&in.desc, L);
  if (out->rc != RNB_OK) { out->error = last_error(); return false; }
  if ((in.parts.albedo || in.parts.feat) && L->F <= 0) { out->rc = RNB_E_INVALID; out->error = "model has no feature head"; return false; }
  Carver c((void*)kFakeWorkspace, (size_t)1 << 43);
  carve_points(*L, c, in.M, in.mode, pb);
  if ((in.parts.albedo && L->route.color == COLOR_H2 && pb->col_part == nullptr) || (in.parts.sdf && in.slabs > 0 && pb->sdfh_part == nullptr)) {
    out->rc = RNB_E_WORKSPACE;
    out->error = "backward: this workspace lacks a buffer the model's kernel route needs";
    return false;
  }
  return true;
}

}  // namespace rnb
