// C-ABI entry points of librnbneus_hip.so (declared in include/rnbneus.h).
#include <math.h>
#include <stdlib.h>

#include "rnb_internal.h"

using namespace rnb;

#define RNB_API extern "C" __attribute__((visibility("default")))

#define RNB_REQUIRE(p, name) \
  if (!(p)) RNB_FAIL(RNB_E_NULL, name " is NULL")

#if __has_include("../build/build_id.h")
#include "../build/build_id.h"   // written by __graft_entry__.build_native: hash of csrc/, include/ and the compiler flags
#endif
#ifndef RNB_BUILD_ID
#define RNB_BUILD_ID "unknown"
#endif

RNB_API int rnb_abi_version(void) { return RNB_ABI_VERSION; }
RNB_API const char* rnb_build_id(void) { return RNB_BUILD_ID; }
RNB_API const char* rnb_last_error_string(void) { return rnb::last_error(); }

RNB_API int rnb_packed_floats(const rnb_model_desc* desc, int64_t* n_floats) {
  RNB_REQUIRE(n_floats, "n_floats");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  *n_floats = L.total_all;
  return RNB_OK;
}

RNB_API int rnb_weightnorm_fwd(const rnb_model_desc* desc, const rnb_mlp_params* sdf, const rnb_mlp_params* color,
                               float* packed, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  RNB_TRY(weightnorm_fwd(desc, L, sdf, color, packed, (hipStream_t)stream));
  if (is_bf16(L)) RNB_TRY(bf16_pack_weights(L, packed, (hipStream_t)stream));   // bf16 mirror behind the fp32 weights
  if (is_x3(L)) RNB_TRY(x3_pack_weights(L, packed, (hipStream_t)stream));       // hi / mid / lo mirror
  return RNB_OK;
}

RNB_API int rnb_weightnorm_bwd(const rnb_model_desc* desc, const rnb_mlp_params* sdf, const rnb_mlp_params* color,
                               const float* packed_grad, const rnb_mlp_grads* sdf_grads,
                               const rnb_mlp_grads* color_grads, rnb_stream_t stream) {
  RNB_REQUIRE(packed_grad, "packed_grad");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  return weightnorm_bwd(desc, L, sdf, color, packed_grad, sdf_grads, color_grads, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------
// point-wise evaluation
// ---------------------------------------------------------------------------------------------------
static const int kPointsMode = PM_WITH_NORMAL | PM_WITH_COLOR;

RNB_API int rnb_points_workspace_bytes(const rnb_model_desc* desc, int64_t n_points, int64_t* bytes) {
  RNB_REQUIRE(bytes, "bytes");
  if (n_points < 0) RNB_FAIL(RNB_E_INVALID, "n_points < 0");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  Carver c(nullptr, 0);
  PointBufs pb;
  carve_points(L, c, n_points, kPointsMode, &pb);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

static int points_setup(const rnb_model_desc* desc, int64_t n, void* ws, size_t ws_bytes, Layout* L, PointBufs* pb) {
  RNB_TRY(make_layout(desc, L));
  RNB_REQUIRE(ws, "workspace");
  Carver c(ws, ws_bytes);
  carve_points(*L, c, n, kPointsMode, pb);
  if (!c.ok) RNB_FAIL(RNB_E_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
  pb->smax = nullptr;   // (state maxima are kept for a render's backward only: nothing zeroes them here)
  return RNB_OK;
}

// The three sweeps of a point batch, each on the model's kernel route (Layout::route).
// positional encoding + forward sweep.  reverse_follows: the caller runs reverse_points next (the per-layer chain's
// forward then leaves the reverse sweep's seed; the fused sweeps seed themselves from D_last).
static int forward_points(const Layout& L, const float* packed, const float* pts, int64_t n, PointBufs& pb,
                          bool save, bool need_feat, bool reverse_follows, float* feat_dense, hipStream_t s) {
  switch (L.route.sdf) {
    case SDF_BF16:
      // (a saved forward whose albedo net is bf16 too: the feature head writes bf16 K8 straight into that net's input)
      RNB_TRY(bf16_forward(L, packed, pts, n, pb, save, need_feat, s, nullptr, save && need_feat && L.route.color == COLOR_BF16));
      break;
    case SDF_FUSED:
      RNB_TRY(fused_forward(L, packed, pts, n, pb, save, need_feat, s));
      break;
    case SDF_LAYERS:
      RNB_TRY(launch_pe_points(L, pts, n, pb, s));
      return sweep_forward(L, packed, pb, need_feat, reverse_follows, feat_dense, s);
  }
  if (need_feat && feat_dense) RNB_TRY(launch_copy_cols(pb.cin, L.Cinp, L.F, n, feat_dense, s));
  return RNB_OK;
}

// reverse-mode normal.  store_ge: also keep d sdf / d e in pb.ge (the Hessian term of the point adjoint; the per-layer
// chain always leaves it, the bf16 route has no input adjoints)
static int reverse_points(const Layout& L, const float* packed, PointBufs& pb, bool store_ge, hipStream_t s) {
  switch (L.route.sdf) {
    case SDF_BF16: return bf16_reverse(L, packed, pb, s);
    case SDF_FUSED: return fused_reverse(L, packed, pb, s, store_ge);
    case SDF_LAYERS: break;
  }
  return sweep_reverse(L, packed, pb, s);
}

// albedo network on the state the two sweeps above left (features in pb.cin / cin8, normals in pb.nrm [Mp,4])
static int color_points(const Layout& L, const float* packed, PointBufs& pb, const float* pts, hipStream_t s) {
  switch (L.route.color) {
    case COLOR_BF16: return bf16_color_forward(L, packed, pb, pts, s);
    case COLOR_H2: return color_h2_forward(L, packed, pb, pts, pb.nrm, s);
    case COLOR_LAYERS: return sweep_color(L, packed, pb, pts, pb.nrm, 4, s);
    case COLOR_NONE: break;
  }
  RNB_FAIL(RNB_E_INVALID, "model has no albedo network");
}

RNB_API int rnb_sdf_forward(const rnb_model_desc* desc, const float* packed, const float* pts, int64_t n,
                            float* sdf_out, float* feat_out, void* ws, size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(pts, "pts");
  RNB_REQUIRE(sdf_out, "sdf_out");
  if (n <= 0) return n == 0 ? RNB_OK : (set_error("n < 0"), RNB_E_INVALID);
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  PointBufs pb;
  RNB_TRY(points_setup(desc, n, ws, ws_bytes, &L, &pb));
  RNB_TRY(forward_points(L, packed, pts, n, pb, false, feat_out != nullptr, false, feat_out, s));
  RNB_CHECK_HIP(hipMemcpyAsync(sdf_out, pb.sdf, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return RNB_OK;
}

RNB_API int rnb_sdf_gradient(const rnb_model_desc* desc, const float* packed, const float* pts, int64_t n,
                             float* grad_out, float* sdf_out, void* ws, size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(pts, "pts");
  RNB_REQUIRE(grad_out, "grad_out");
  if (n <= 0) return n == 0 ? RNB_OK : (set_error("n < 0"), RNB_E_INVALID);
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  PointBufs pb;
  RNB_TRY(points_setup(desc, n, ws, ws_bytes, &L, &pb));
  RNB_TRY(forward_points(L, packed, pts, n, pb, true, false, true, nullptr, s));
  RNB_TRY(reverse_points(L, packed, pb, false, s));
  RNB_TRY(launch_copy_cols(pb.nrm, 4, 3, n, grad_out, s));
  if (sdf_out) RNB_CHECK_HIP(hipMemcpyAsync(sdf_out, pb.sdf, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return RNB_OK;
}

RNB_API int rnb_color_forward(const rnb_model_desc* desc, const float* packed, const float* pts, const float* normals,
                              const float* feats, int64_t n, float* out, void* ws, size_t ws_bytes,
                              rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(pts, "pts");
  RNB_REQUIRE(normals, "normals");
  RNB_REQUIRE(feats, "feats");
  RNB_REQUIRE(out, "out");
  if (n <= 0) return n == 0 ? RNB_OK : (set_error("n < 0"), RNB_E_INVALID);
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  PointBufs pb;
  RNB_TRY(points_setup(desc, n, ws, ws_bytes, &L, &pb));
  if (L.F <= 0) RNB_FAIL(RNB_E_INVALID, "model has no feature head");
  RNB_TRY(launch_fill_cols(feats, L.F, n, pb.Mp, L.Cinp, pb.cin, s));
  // (always the per-layer chain, whatever the route: it alone reads the caller's dense [n,3] normals and fp32 features)
  RNB_TRY(sweep_color(L, packed, pb, pts, normals, 3, s));
  RNB_TRY(launch_copy_cols(pb.alb, 4, L.Co, n, out, s));
  return RNB_OK;
}

// ---------------------------------------------------------------------------------------------------
// point-wise autograd of the direct network calls (SDFNetwork.forward / .sdf / .gradient, RenderingNetwork.forward)
// ---------------------------------------------------------------------------------------------------
// What the forward keeps is the render path's per-point state (carve_points with PM_WITH_BACKWARD); without the normal
// neither gz_l nor u_l is carved (PM_NO_REVERSE).  The backward is sweep_backward_parts below the composite.
static int grad_mode(int32_t flags) {
  int mode = PM_WITH_BACKWARD | ((flags & RNB_POINTS_NORMAL) ? PM_WITH_NORMAL : PM_NO_REVERSE);
  if (flags & (RNB_POINTS_FEATURE | RNB_POINTS_COLOR)) mode |= PM_WITH_COLOR;
  return mode;
}

static int check_points_flags(int32_t flags) {
  if (flags & ~(RNB_POINTS_FEATURE | RNB_POINTS_NORMAL | RNB_POINTS_COLOR))
    RNB_FAIL(RNB_E_INVALID, "unknown bits in the point-call flags (0x%x)", flags);
  return RNB_OK;
}

RNB_API int rnb_points_grad_workspace_bytes(const rnb_model_desc* desc, int64_t n_points, int32_t flags, int64_t* bytes) {
  RNB_REQUIRE(bytes, "bytes");
  if (n_points < 0) RNB_FAIL(RNB_E_INVALID, "n_points < 0");
  RNB_TRY(check_points_flags(flags));
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  Carver c(nullptr, 0);
  PointBufs pb;
  carve_points(L, c, n_points, grad_mode(flags), &pb);
  Carver cf(nullptr, 0);   // (never below the forward-only calls' workspace: one buffer serves both)
  carve_points(L, cf, n_points, kPointsMode, &pb);
  *bytes = (int64_t)(c.off > cf.off ? c.off : cf.off);
  return RNB_OK;
}

static int grad_setup(const rnb_model_desc* desc, int64_t n, int32_t flags, void* ws, size_t ws_bytes, Layout* L,
                      PointBufs* pb) {
  RNB_TRY(check_points_flags(flags));
  RNB_TRY(make_layout(desc, L));
  if (is_bf16(*L)) RNB_FAIL(RNB_E_INVALID, "RNB_VARIANT_BF16 has no point-wise backward (the render path only)");
  if ((flags & (RNB_POINTS_FEATURE | RNB_POINTS_COLOR)) && L->F <= 0) RNB_FAIL(RNB_E_INVALID, "model has no feature head");
  RNB_REQUIRE(ws, "workspace");
  Carver c(ws, ws_bytes);
  carve_points(*L, c, n, grad_mode(flags), pb);
  if (!c.ok) RNB_FAIL(RNB_E_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
  return RNB_OK;
}

RNB_API int rnb_sdf_forward_save(const rnb_model_desc* desc, const float* packed, const float* pts, int64_t n,
                                 int32_t flags, float* sdf_out, float* feat_out, float* nrm_out, void* ws,
                                 size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(pts, "pts");
  RNB_REQUIRE(sdf_out, "sdf_out");
  if (flags & RNB_POINTS_COLOR) RNB_FAIL(RNB_E_INVALID, "RNB_POINTS_COLOR belongs to rnb_color_forward_save");
  const bool feat = (flags & RNB_POINTS_FEATURE) != 0, normal = (flags & RNB_POINTS_NORMAL) != 0;
  if (feat) RNB_REQUIRE(feat_out, "feat_out");
  if (normal) RNB_REQUIRE(nrm_out, "nrm_out");
  if (n <= 0) return n == 0 ? RNB_OK : (set_error("n < 0"), RNB_E_INVALID);
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  PointBufs pb;
  RNB_TRY(grad_setup(desc, n, flags, ws, ws_bytes, &L, &pb));
  // state maxima of the x2h weight-gradient jobs: zeroed here (a render's first kernel does it there), grown by the sweeps
  RNB_CHECK_HIP(hipMemsetAsync(pb.smax, 0, SMAX_SLOTS * sizeof(unsigned), s));
  RNB_TRY(forward_points(L, packed, pts, n, pb, true, feat, normal, feat ? feat_out : nullptr, s));
  if (normal) {
    RNB_TRY(reverse_points(L, packed, pb, true, s));   // (+ d sdf / d e for the Hessian term of x's adjoint)
    RNB_TRY(launch_copy_cols(pb.nrm, 4, 3, n, nrm_out, s));
  }
  RNB_CHECK_HIP(hipMemcpyAsync(sdf_out, pb.sdf, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return RNB_OK;
}

RNB_API int rnb_sdf_backward(const rnb_model_desc* desc, const float* packed, int64_t n, int32_t flags,
                             const float* sdf_bar, const float* feat_bar, const float* nrm_bar, float* packed_grad,
                             float* x_bar, void* ws, size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(packed_grad, "packed_grad");
  if (feat_bar && !(flags & RNB_POINTS_FEATURE)) RNB_FAIL(RNB_E_INVALID, "feat_bar without RNB_POINTS_FEATURE");
  if (nrm_bar && !(flags & RNB_POINTS_NORMAL)) RNB_FAIL(RNB_E_INVALID, "nrm_bar without RNB_POINTS_NORMAL");
  if (flags & RNB_POINTS_COLOR) RNB_FAIL(RNB_E_INVALID, "RNB_POINTS_COLOR belongs to rnb_color_backward");
  if (n < 0) RNB_FAIL(RNB_E_INVALID, "n < 0");
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  RNB_CHECK_HIP(hipMemsetAsync(packed_grad, 0, (size_t)L.total * sizeof(float), s));
  if (n == 0) return RNB_OK;
  PointBufs pb;
  RNB_TRY(grad_setup(desc, n, flags, ws, ws_bytes, &L, &pb));
  const int64_t Mp = pb.Mp;
  // the adjoints' maxima: zeroed (composite_bwd_kernel's job in a render), then grown by every producer; the caller's
  // feature adjoint is one of them (the feature head's weight-gradient job reads its slot)
  RNB_CHECK_HIP(hipMemsetAsync(pb.amax, 0, AMAX_SLOTS * sizeof(unsigned), s));
  RNB_CHECK_HIP(hipMemsetAsync(pb.sbar, 0, (size_t)Mp * sizeof(float), s));
  if (sdf_bar) RNB_CHECK_HIP(hipMemcpyAsync(pb.sbar, sdf_bar, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (nrm_bar) {
    RNB_CHECK_HIP(hipMemsetAsync(pb.nbar, 0, (size_t)Mp * 4 * sizeof(float), s));
    RNB_TRY(launch_fill_cols(nrm_bar, 3, n, Mp, 4, pb.nbar, s));
  }
  if (feat_bar) {
    RNB_CHECK_HIP(hipMemsetAsync(pb.cinb, 0, (size_t)Mp * L.Cinp * sizeof(float), s));
    RNB_TRY(launch_fill_cols(feat_bar, L.F, n, Mp, L.Cinp, pb.cinb, s));
    if (L.route.h2) RNB_TRY(launch_absmax_rows(pb.cinb, Mp * L.Cinp, pb.amax + AMAX_CINB, s));
  }
  RNB_TRY(sweep_backward_parts(L, packed, pb, BwdParts::sdf_points(feat_bar != nullptr, nrm_bar != nullptr), packed_grad, s));
  if (x_bar) RNB_TRY(launch_sdf_xbar(L, packed, pb, nrm_bar != nullptr, x_bar, s));
  return RNB_OK;
}

RNB_API int rnb_color_forward_save(const rnb_model_desc* desc, const float* packed, const float* pts,
                                   const float* normals, const float* feats, int64_t n, float* out, void* ws,
                                   size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(pts, "pts");
  RNB_REQUIRE(normals, "normals");
  RNB_REQUIRE(feats, "feats");
  RNB_REQUIRE(out, "out");
  if (n <= 0) return n == 0 ? RNB_OK : (set_error("n < 0"), RNB_E_INVALID);
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  PointBufs pb;
  RNB_TRY(grad_setup(desc, n, RNB_POINTS_COLOR, ws, ws_bytes, &L, &pb));
  const int64_t Mp = pb.Mp;
  // the inputs, kept for the input adjoints: points -> pb.x, normals -> pb.nrm ([Mp,4], zero padding), features -> cin
  RNB_CHECK_HIP(hipMemsetAsync(pb.x, 0, (size_t)Mp * 4 * sizeof(float), s));
  RNB_CHECK_HIP(hipMemsetAsync(pb.nrm, 0, (size_t)Mp * 4 * sizeof(float), s));
  RNB_CHECK_HIP(hipMemsetAsync(pb.smax, 0, SMAX_SLOTS * sizeof(unsigned), s));
  RNB_TRY(launch_fill_cols(pts, 3, n, Mp, 4, pb.x, s));
  RNB_TRY(launch_fill_cols(normals, 3, n, Mp, 4, pb.nrm, s));
  RNB_TRY(launch_fill_cols(feats, L.F, n, Mp, L.Cinp, pb.cin, s));
  RNB_TRY(color_points(L, packed, pb, pts, s));
  RNB_TRY(launch_copy_cols(pb.alb, 4, L.Co, n, out, s));
  return RNB_OK;
}

RNB_API int rnb_color_backward(const rnb_model_desc* desc, const float* packed, int64_t n, const float* alb_bar,
                               float* packed_grad, float* feat_bar, float* nrm_bar, float* pts_bar, void* ws,
                               size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(alb_bar, "alb_bar");
  RNB_REQUIRE(packed_grad, "packed_grad");
  if (n < 0) RNB_FAIL(RNB_E_INVALID, "n < 0");
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  RNB_CHECK_HIP(hipMemsetAsync(packed_grad, 0, (size_t)L.total * sizeof(float), s));
  if (n == 0) return RNB_OK;
  PointBufs pb;
  RNB_TRY(grad_setup(desc, n, RNB_POINTS_COLOR, ws, ws_bytes, &L, &pb));
  const int64_t Mp = pb.Mp;
  RNB_CHECK_HIP(hipMemsetAsync(pb.amax, 0, AMAX_SLOTS * sizeof(unsigned), s));
  RNB_CHECK_HIP(hipMemsetAsync(pb.albbar, 0, (size_t)Mp * 4 * sizeof(float), s));
  RNB_TRY(launch_fill_cols(alb_bar, L.Co, n, Mp, 4, pb.albbar, s));
  RNB_TRY(sweep_backward_parts(L, packed, pb, BwdParts::color_points(pts_bar != nullptr || nrm_bar != nullptr), packed_grad, s));
  if (feat_bar) RNB_TRY(launch_copy_cols(pb.cinb, L.Cinp, L.F, n, feat_bar, s));
  RNB_TRY(launch_color_input_bwd(L, pb, pts_bar, nrm_bar, s));
  return RNB_OK;
}

// ---------------------------------------------------------------------------------------------------
// per-vertex mesh attributes (validate_mesh_texture): kernels in mesh_attrs.hip
// ---------------------------------------------------------------------------------------------------
struct MeshBufs {
  float* pts;     // [chunk,3] the chunk's points (the Newton steps move them in place)
  PointBufs pb;   // per-point state of `chunk` points: a forward-only render's (normal + colour)
};

static int check_mesh_chunk(int64_t chunk, int32_t flags) {
  if (chunk <= 0 || chunk % 64 != 0) RNB_FAIL(RNB_E_INVALID, "mesh vertices: chunk must be a positive multiple of 64 (%lld)", (long long)chunk);
  if (flags & ~(RNB_MESH_ALBEDO | RNB_MESH_SWAP_RB)) RNB_FAIL(RNB_E_INVALID, "mesh vertices: unknown flag bits (0x%x)", flags);
  return RNB_OK;
}

static void carve_mesh(const Layout& L, Carver& c, int64_t chunk, MeshBufs* mb) {
  mb->pts = c.take<float>(chunk * 3);
  carve_points(L, c, chunk, kPointsMode, &mb->pb);
}

RNB_API int rnb_mesh_vertex_workspace_bytes(const rnb_model_desc* desc, int64_t chunk, int32_t flags, int64_t* bytes) {
  RNB_REQUIRE(bytes, "bytes");
  RNB_TRY(check_mesh_chunk(chunk, flags));
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  if ((flags & RNB_MESH_ALBEDO) && L.route.color == COLOR_NONE) RNB_FAIL(RNB_E_INVALID, "mesh vertices: RNB_MESH_ALBEDO on a model without an albedo network");
  Carver c(nullptr, 0);
  MeshBufs mb;
  carve_mesh(L, c, chunk, &mb);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

RNB_API int rnb_mesh_vertex_attrs(const rnb_model_desc* desc, const float* packed, const rnb_mesh_vertex_args* a,
                                  int64_t chunk, void* ws, size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(a, "args");
  RNB_TRY(check_mesh_chunk(chunk, a->flags));
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  const bool albedo = (a->flags & RNB_MESH_ALBEDO) != 0;
  if (albedo && L.route.color == COLOR_NONE) RNB_FAIL(RNB_E_INVALID, "mesh vertices: RNB_MESH_ALBEDO on a model without an albedo network");
  if (!albedo && (a->albedo_out || a->rgb_out)) RNB_FAIL(RNB_E_INVALID, "mesh vertices: albedo_out / rgb_out without RNB_MESH_ALBEDO");
  if (a->rgb_out && L.Co != 1 && L.Co != 3) RNB_FAIL(RNB_E_INVALID, "mesh vertices: rgb_out needs col_d_out 1 or 3 (%d)", L.Co);
  if (a->refine < 0) RNB_FAIL(RNB_E_INVALID, "mesh vertices: refine < 0");
  if (a->refine > 0 && !(a->max_step > 0.f)) RNB_FAIL(RNB_E_INVALID, "mesh vertices: refine > 0 needs max_step > 0 (%g)", (double)a->max_step);
  if (a->V < 0) RNB_FAIL(RNB_E_INVALID, "mesh vertices: V < 0");
  if (!(a->points_out || a->sdf_out || a->gradient_out || a->normal_out || a->albedo_out || a->rgb_out))
    RNB_FAIL(RNB_E_INVALID, "mesh vertices: no output requested (every output pointer is NULL)");
  if (a->grid_vertices && a->resolution < 2) RNB_FAIL(RNB_E_INVALID, "mesh vertices: grid_vertices of a resolution %d grid", a->resolution);
  if (a->V == 0) return RNB_OK;
  if (!a->grid_vertices) RNB_REQUIRE(a->points, "grid_vertices and points");
  RNB_REQUIRE(ws, "workspace");
  Carver c(ws, ws_bytes);
  MeshBufs mb;
  carve_mesh(L, c, chunk, &mb);
  if (!c.ok) RNB_FAIL(RNB_E_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
  MeshPointsSrc src;
  memset(&src, 0, sizeof(src));
  src.grid = a->grid_vertices;
  src.pts = a->points;
  src.rm1 = (double)a->resolution - 1.0;
  for (int d = 0; d < 3; ++d) {
    src.span[d] = a->bound_max[d] - a->bound_min[d];   // fp32, as the host's numpy does it
    src.bmin[d] = a->bound_min[d];
  }
  MeshOut o;
  memset(&o, 0, sizeof(o));
  o.points = a->points_out; o.sdf = a->sdf_out; o.gradient = a->gradient_out; o.normal = a->normal_out;
  o.albedo = a->albedo_out; o.rgb = a->rgb_out;
  o.Co = L.Co;
  o.swap_rb = (a->flags & RNB_MESH_SWAP_RB) ? 1 : 0;
  // the state maxima of a saved forward, as a forward-only render keeps them (zeroed once: they only grow, nothing reads them)
  RNB_CHECK_HIP(hipMemsetAsync(mb.pb.smax, 0, SMAX_SLOTS * sizeof(unsigned), s));
  // every chunk through the one workspace: its kernels are enqueued behind the previous chunk's (stream order)
  for (int64_t first = 0; first < a->V; first += chunk) {
    const int64_t m = a->V - first < chunk ? a->V - first : chunk;
    PointBufs pb = mb.pb;
    pb.M = m;
    pb.Mp = pad_rows(m);
    RNB_TRY(launch_mesh_points(src, first, m, mb.pts, s));
    for (int step = 0; step <= a->refine; ++step) {
      if (step > 0) RNB_TRY(launch_mesh_newton(pb.sdf, pb.nrm, m, a->level, a->max_step, mb.pts, s));
      // (the features feed the albedo network alone: only the sweep at the final points writes them)
      RNB_TRY(forward_points(L, packed, mb.pts, m, pb, true, albedo && step == a->refine, true, nullptr, s));
      RNB_TRY(reverse_points(L, packed, pb, false, s));
    }
    if (albedo) RNB_TRY(color_points(L, packed, pb, mb.pts, s));
    RNB_TRY(launch_mesh_attrs(mb.pts, pb, first, m, o, s));
  }
  return RNB_OK;
}

// ---------------------------------------------------------------------------------------------------
// SDF grid (extract_fields)
// ---------------------------------------------------------------------------------------------------
constexpr int64_t kGridChunk = 1 << 20;   // points per pass of the generic (per-layer GEMM) path

static int check_grid(const rnb_grid_desc* gd, int64_t* n_points) {
  RNB_REQUIRE(gd, "grid");
  if (gd->resolution < 1 || gd->resolution > 4096) RNB_FAIL(RNB_E_INVALID, "grid resolution out of range (%d)", gd->resolution);
  if (gd->x_begin < 0 || gd->x_end > gd->resolution || gd->x_begin > gd->x_end)
    RNB_FAIL(RNB_E_INVALID, "bad x-slab [%d, %d) of a %d grid", gd->x_begin, gd->x_end, gd->resolution);
  *n_points = (int64_t)(gd->x_end - gd->x_begin) * gd->resolution * gd->resolution;
  return RNB_OK;
}

static GridGen grid_gen_of(const rnb_grid_desc* gd) {
  GridGen g;
  memset(&g, 0, sizeof(g));
  g.on = GRID_DENSE;
  g.res = gd->resolution;
  g.x_begin = gd->x_begin;
  for (int d = 0; d < 3; ++d) { g.bmin[d] = gd->bound_min[d]; g.bmax[d] = gd->bound_max[d]; }
  g.out_scale = gd->out_scale;
  return g;
}

RNB_API int rnb_sdf_grid_workspace_bytes(const rnb_model_desc* desc, const rnb_grid_desc* grid, int64_t* bytes) {
  RNB_REQUIRE(bytes, "bytes");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  int64_t n;
  RNB_TRY(check_grid(grid, &n));
  if (L.route.sdf != SDF_LAYERS) { *bytes = 256; return RNB_OK; }   // the fused sweeps keep everything in LDS
  Carver c(nullptr, 0);
  PointBufs pb;
  c.take<float>(kGridChunk * 3);
  carve_points(L, c, n < kGridChunk ? n : kGridChunk, PM_SDF_ONLY, &pb);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

RNB_API int rnb_sdf_grid(const rnb_model_desc* desc, const float* packed, const rnb_grid_desc* grid, float* volume,
                         void* ws, size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(volume, "volume");
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  int64_t n;
  RNB_TRY(check_grid(grid, &n));
  if (n == 0) return RNB_OK;
  const GridGen gg = grid_gen_of(grid);
  if (L.route.sdf != SDF_LAYERS) {   // the grid points are generated inside the forward kernel
    PointBufs pb;
    memset(&pb, 0, sizeof(pb));
    pb.M = n;
    pb.Mp = pad_rows(n);
    pb.sdf = volume;   // grid mode writes rows < M only
    if (L.route.sdf == SDF_BF16) return bf16_forward(L, packed, nullptr, n, pb, false, false, s, &gg);
    return fused_forward(L, packed, nullptr, n, pb, false, false, s, &gg);
  }
  RNB_REQUIRE(ws, "workspace");
  for (int64_t first = 0; first < n; first += kGridChunk) {
    const int64_t m = n - first < kGridChunk ? n - first : kGridChunk;
    Carver c(ws, ws_bytes);
    float* pts = c.take<float>(kGridChunk * 3);
    PointBufs pb;
    carve_points(L, c, n < kGridChunk ? n : kGridChunk, PM_SDF_ONLY, &pb);
    if (!c.ok) RNB_FAIL(RNB_E_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
    pb.M = m;
    pb.Mp = pad_rows(m);
    RNB_TRY(launch_grid_points(gg, first, m, pts, s));
    RNB_TRY(forward_points(L, packed, pts, m, pb, false, false, false, nullptr, s));
    RNB_TRY(launch_scale_copy(pb.sdf, gg.out_scale, m, volume + first, s));
  }
  return RNB_OK;
}

// ---------------------------------------------------------------------------------------------------
// sparse SDF grid: the bricks near the surface only (kernels: sparse_grid.hip + the brick mode of the forward sweeps)
// ---------------------------------------------------------------------------------------------------
constexpr int64_t kSparseRowsPerLaunch = (int64_t)1 << 28;   // rows of one brick-mode sweep (its block count fits 32 bits)

struct SparseSetup {
  Layout L;
  GridGen gg;          // the dense grid's generator + brick geometry (on is set per sweep)
  SparseGeom sg;
  float* lattice;      // [nl^3] values at the brick corners
  uint32_t* state;     // [ceil(nb^3 / 4)] one byte per brick
  int32_t* list;       // [nb^3] listed bricks
  float* pts;          // per-layer route: points of one chunk, and the chunk's buffers
  PointBufs pb;
};

// checks + workspace carving shared by the four entry points (ws == nullptr: sizing only)
static int sparse_setup(const rnb_model_desc* desc, const rnb_grid_desc* grid, const rnb_sparse_grid_desc* sp, void* ws,
                        size_t ws_bytes, SparseSetup* S, size_t* need) {
  RNB_REQUIRE(sp, "sparse");
  RNB_TRY(make_layout(desc, &S->L));
  int64_t n;
  RNB_TRY(check_grid(grid, &n));
  const int res = grid->resolution, bs = sp->brick;
  if (res < 2) RNB_FAIL(RNB_E_INVALID, "sparse grid: resolution %d has no cells", res);
  if (grid->x_begin != 0 || grid->x_end != res)
    RNB_FAIL(RNB_E_INVALID, "sparse grid: x-slab [%d, %d) is not the whole %d grid (use rnb_sdf_grid for slabs)", grid->x_begin,
             grid->x_end, res);
  if (bs != 4 && bs != 8 && bs != 16 && bs != 32) RNB_FAIL(RNB_E_INVALID, "sparse grid: brick must be 4, 8, 16 or 32 (%d)", bs);
  if (!(sp->margin >= 0.f)) RNB_FAIL(RNB_E_INVALID, "sparse grid: margin must be >= 0 (%g)", (double)sp->margin);
  if (sp->threshold != sp->threshold) RNB_FAIL(RNB_E_INVALID, "sparse grid: threshold is NaN");
  const int nb = (res - 1 + bs - 1) / bs, nl = nb + 1;
  const int64_t nbr = (int64_t)nb * nb * nb;
  if (nbr > INT32_MAX) RNB_FAIL(RNB_E_INVALID, "sparse grid: %lld bricks do not fit a 32-bit id", (long long)nbr);
  S->gg = grid_gen_of(grid);
  S->gg.bs = bs;
  S->gg.nb = nb;
  S->gg.rows_per_brick = ((bs + 1) * (bs + 1) * (bs + 1) + 63) / 64 * 64;
  S->gg.family_rows = pad_rows(n);
  double diag2 = 0;
  for (int d = 0; d < 3; ++d) {
    const double edge = ((double)grid->bound_max[d] - (double)grid->bound_min[d]) / (res - 1) * bs;
    diag2 += edge * edge;
  }
  S->sg.res = res; S->sg.bs = bs; S->sg.nb = nb; S->sg.nl = nl;
  S->sg.thr = sp->threshold;
  // (the volume holds out_scale * sdf: a Lipschitz constant `margin` of the SDF is margin * |out_scale| of the values)
  S->sg.seed_dist = (float)((double)sp->margin * fabs((double)grid->out_scale) * 0.5 * sqrt(diag2));
  Carver c(ws, ws_bytes);
  S->lattice = c.take<float>((int64_t)nl * nl * nl);
  S->state = c.take<uint32_t>((nbr + 3) / 4);
  S->list = c.take<int32_t>(nbr);
  S->pts = nullptr;
  if (S->L.route.sdf == SDF_LAYERS) {   // the fused sweeps keep everything in LDS
    S->pts = c.take<float>(kGridChunk * 3);
    carve_points(S->L, c, kGridChunk, PM_SDF_ONLY, &S->pb);
  }
  *need = c.off;
  if (ws == nullptr) return RNB_OK;
  if (!c.ok) RNB_FAIL(RNB_E_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
  return RNB_OK;
}

// rows [0, M) of the grid generator g (brick list or lattice) through the model's forward route, values to `out`
static int sparse_eval(SparseSetup& S, const float* packed, const GridGen& g, int64_t M, float* out, hipStream_t s) {
  if (S.L.route.sdf != SDF_LAYERS) {
    PointBufs pb;
    memset(&pb, 0, sizeof(pb));
    pb.M = M;
    pb.Mp = pad_rows(M);
    pb.sdf = out;
    if (S.L.route.sdf == SDF_BF16) return bf16_forward(S.L, packed, nullptr, M, pb, false, false, s, &g);
    return fused_forward(S.L, packed, nullptr, M, pb, false, false, s, &g);
  }
  for (int64_t first = 0; first < M; first += kGridChunk) {
    const int64_t m = M - first < kGridChunk ? M - first : kGridChunk;
    PointBufs pb = S.pb;
    pb.M = m;
    pb.Mp = pad_rows(m);
    RNB_TRY(launch_grid_points(g, first, m, S.pts, s));
    RNB_TRY(forward_points(S.L, packed, S.pts, m, pb, false, false, false, nullptr, s));
    RNB_TRY(launch_grid_scatter(g, pb.sdf, first, m, out, s));
  }
  return RNB_OK;
}

RNB_API int rnb_sdf_grid_sparse_workspace_bytes(const rnb_model_desc* desc, const rnb_grid_desc* grid,
                                                const rnb_sparse_grid_desc* sparse, int64_t* bytes) {
  RNB_REQUIRE(bytes, "bytes");
  SparseSetup S;
  size_t need = 0;
  RNB_TRY(sparse_setup(desc, grid, sparse, nullptr, 0, &S, &need));
  *bytes = (int64_t)need;
  return RNB_OK;
}

RNB_API int rnb_sdf_grid_sparse_seed(const rnb_model_desc* desc, const float* packed, const rnb_grid_desc* grid,
                                     const rnb_sparse_grid_desc* sparse, void* ws, size_t ws_bytes, int64_t* n_listed,
                                     rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(ws, "workspace");
  RNB_REQUIRE(n_listed, "n_listed");
  hipStream_t s = (hipStream_t)stream;
  SparseSetup S;
  size_t need = 0;
  RNB_TRY(sparse_setup(desc, grid, sparse, ws, ws_bytes, &S, &need));
  RNB_CHECK_HIP(hipMemsetAsync(n_listed, 0, sizeof(int64_t), s));
  GridGen g = S.gg;
  g.on = GRID_LATTICE;
  RNB_TRY(sparse_eval(S, packed, g, (int64_t)S.sg.nl * S.sg.nl * S.sg.nl, S.lattice, s));
  return launch_sparse_classify(S.sg, S.lattice, S.state, S.list, n_listed, s);
}

RNB_API int rnb_sdf_grid_sparse_round(const rnb_model_desc* desc, const float* packed, const rnb_grid_desc* grid,
                                      const rnb_sparse_grid_desc* sparse, float* volume, void* ws, size_t ws_bytes,
                                      int64_t first, int64_t count, int64_t* n_listed, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(volume, "volume");
  RNB_REQUIRE(ws, "workspace");
  RNB_REQUIRE(n_listed, "n_listed");
  hipStream_t s = (hipStream_t)stream;
  SparseSetup S;
  size_t need = 0;
  RNB_TRY(sparse_setup(desc, grid, sparse, ws, ws_bytes, &S, &need));
  const int64_t nbr = (int64_t)S.sg.nb * S.sg.nb * S.sg.nb;
  if (first < 0 || count < 0 || first + count > nbr)
    RNB_FAIL(RNB_E_INVALID, "sparse grid: bricks [%lld, %lld) of a list of at most %lld", (long long)first,
             (long long)(first + count), (long long)nbr);
  if (count == 0) return RNB_OK;
  GridGen g = S.gg;
  g.on = GRID_BRICKS;
  const int64_t per = kSparseRowsPerLaunch / g.rows_per_brick;   // bricks per sweep
  for (int64_t at = 0; at < count; at += per) {
    const int64_t nbk = count - at < per ? count - at : per;
    g.bricks = S.list + first + at;
    RNB_TRY(sparse_eval(S, packed, g, nbk * g.rows_per_brick, volume, s));
  }
  return launch_sparse_grow(S.sg, volume, first, count, S.state, S.list, n_listed, s);
}

RNB_API int rnb_sdf_grid_sparse_finish(const rnb_model_desc* desc, const rnb_grid_desc* grid,
                                       const rnb_sparse_grid_desc* sparse, float* volume, void* ws, size_t ws_bytes,
                                       uint8_t* brick_mask, rnb_stream_t stream) {
  RNB_REQUIRE(volume, "volume");
  RNB_REQUIRE(ws, "workspace");
  hipStream_t s = (hipStream_t)stream;
  SparseSetup S;
  size_t need = 0;
  RNB_TRY(sparse_setup(desc, grid, sparse, ws, ws_bytes, &S, &need));
  RNB_TRY(launch_sparse_fill(S.sg, S.lattice, S.state, volume, s));
  if (brick_mask)
    RNB_CHECK_HIP(hipMemcpyAsync(brick_mask, S.state, (size_t)S.sg.nb * S.sg.nb * S.sg.nb, hipMemcpyDeviceToDevice, s));
  return RNB_OK;
}

// ---------------------------------------------------------------------------------------------------
// hierarchical sampling
// ---------------------------------------------------------------------------------------------------
RNB_API int rnb_up_sample_step(const float* rays_o, const float* rays_d, const float* z_in, const float* sdf_in,
                               int64_t B, int32_t n, int32_t n_new, float inv_s, float* new_z, int32_t* inds,
                               float* z_out, int32_t* sort_index, rnb_stream_t stream) {
  RNB_REQUIRE(rays_o, "rays_o");
  RNB_REQUIRE(rays_d, "rays_d");
  RNB_REQUIRE(z_in, "z_in");
  RNB_REQUIRE(sdf_in, "sdf_in");
  RNB_REQUIRE(z_out, "z_out");
  if (B <= 0) return B == 0 ? RNB_OK : (set_error("B < 0"), RNB_E_INVALID);
  return launch_up_sample_step(rays_o, rays_d, z_in, sdf_in, nullptr, nullptr, n, B, n, n_new, inv_s, new_z, inds,
                               z_out, sort_index, nullptr, nullptr, (hipStream_t)stream);
}

RNB_API int rnb_gather_sdf(const float* sdf_old, const float* sdf_new, const int32_t* sort_index, int64_t B,
                           int32_t n, int32_t n_new, float* sdf_out, rnb_stream_t stream) {
  RNB_REQUIRE(sdf_old, "sdf_old");
  RNB_REQUIRE(sdf_new, "sdf_new");
  RNB_REQUIRE(sort_index, "sort_index");
  RNB_REQUIRE(sdf_out, "sdf_out");
  if (B <= 0) return B == 0 ? RNB_OK : (set_error("B < 0"), RNB_E_INVALID);
  return launch_gather_sdf(sdf_old, sdf_new, sort_index, B, n, n_new, sdf_out, (hipStream_t)stream);
}

struct SampleBufs {
  float* z[2];
  float* sdf[2];
  int32_t* index[2];   // sort index of a step (read by the next step's kernel while that one writes its own: ping-pong)
  float* pts;      // [B*n_samples,3] coarse points, later [B*n_new,3]
  PointBufs pb;    // sized for B*n_samples points
  size_t pb_off;   // carve offset of the point buffers
};

static void carve_sample(const Layout& L, const rnb_model_desc* d, Carver& c, int64_t B, SampleBufs* sb) {
  const int S = d->n_samples + d->n_importance;
  for (int i = 0; i < 2; ++i) sb->z[i] = c.take<float>(B * S);
  for (int i = 0; i < 2; ++i) sb->sdf[i] = c.take<float>(B * S);
  for (int i = 0; i < 2; ++i) sb->index[i] = c.take<int32_t>(B * S);
  sb->pts = c.take<float>(B * d->n_samples * 3);
  sb->pb_off = c.off;
  carve_points(L, c, B * d->n_samples, PM_SDF_ONLY, &sb->pb);
}

static int check_sampling_desc(const rnb_model_desc* d) {
  if (d->n_samples < 2) RNB_FAIL(RNB_E_INVALID, "n_samples must be >= 2");
  if (d->n_importance < 0) RNB_FAIL(RNB_E_INVALID, "n_importance < 0");
  if (d->n_importance > 0) {
    if (d->up_sample_steps < 1 || d->n_importance % d->up_sample_steps != 0)
      RNB_FAIL(RNB_E_INVALID, "n_importance (%d) must be a positive multiple of up_sample_steps (%d)",
               d->n_importance, d->up_sample_steps);
    if (d->n_importance / d->up_sample_steps > d->n_samples)
      RNB_FAIL(RNB_E_INVALID, "n_importance/up_sample_steps must not exceed n_samples");
    // the limits of up_sample_kernel (launch_up_sample_step checks them again per step): refused here, before the
    // workspace query answers and before rnb_sample_rays launches the coarse forward
    if (d->n_importance / d->up_sample_steps > kMaxNew)
      RNB_FAIL(RNB_E_INVALID, "n_importance/up_sample_steps = %d new depths per step > %d (kMaxNew)",
               d->n_importance / d->up_sample_steps, kMaxNew);
    if (d->n_samples + d->n_importance > kMaxZ)
      RNB_FAIL(RNB_E_INVALID, "n_samples + n_importance = %d depths per ray > %d (kMaxZ)",
               d->n_samples + d->n_importance, kMaxZ);
  }
  return RNB_OK;
}

RNB_API int rnb_sample_workspace_bytes(const rnb_model_desc* desc, int64_t B, int64_t* bytes) {
  RNB_REQUIRE(bytes, "bytes");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  RNB_TRY(check_sampling_desc(desc));
  if (B < 0) RNB_FAIL(RNB_E_INVALID, "B < 0");
  Carver c(nullptr, 0);
  SampleBufs sb;
  carve_sample(L, desc, c, B, &sb);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

RNB_API int rnb_sample_rays(const rnb_model_desc* desc, const float* packed, const float* rays_o, const float* rays_d,
                            const float* near, const float* far, const float* t_rand, int64_t B, float* z_vals_out,
                            void* ws, size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(rays_o, "rays_o");
  RNB_REQUIRE(rays_d, "rays_d");
  RNB_REQUIRE(near, "near");
  RNB_REQUIRE(far, "far");
  RNB_REQUIRE(z_vals_out, "z_vals_out");
  if (B <= 0) return B == 0 ? RNB_OK : (set_error("B < 0"), RNB_E_INVALID);
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  RNB_TRY(check_sampling_desc(desc));
  const int n0 = desc->n_samples;
  if (desc->n_importance == 0) return launch_z_init(rays_o, rays_d, near, far, t_rand, B, n0, z_vals_out, nullptr, s);
  RNB_REQUIRE(ws, "workspace");
  Carver c(ws, ws_bytes);
  SampleBufs sb;
  carve_sample(L, desc, c, B, &sb);
  if (!c.ok) RNB_FAIL(RNB_E_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
  const int steps = desc->up_sample_steps;
  const int n_new = desc->n_importance / steps;

  RNB_TRY(launch_z_init(rays_o, rays_d, near, far, t_rand, B, n0, sb.z[0], sb.pts, s));
  RNB_TRY(forward_points(L, packed, sb.pts, B * n0, sb.pb, false, false, false, nullptr, s));
  // The SDF row travels through the loop inside the up-sampling kernel itself (renderer.py:185-190: sdf = cat[sdf,
  // new_sdf] gathered by the sort index): step i reads the row step i - 1 left sorted, the SDF of the points step i - 1
  // proposed and its sort index, and leaves the merged row for step i + 1 — no separate gather launches, no copy of the
  // coarse row out of the point buffers (which the next forward re-carves).
  const float* sdf_old = sb.pb.sdf;    // step 0: the coarse row, as the forward wrote it
  const float* sdf_new = nullptr;
  const int32_t* gidx = nullptr;
  int n_old = n0;
  int cur = 0;
  int n = n0;
  for (int i = 0; i < steps; ++i) {
    const bool last = (i + 1 == steps);
    float* z_next = last ? z_vals_out : sb.z[cur ^ 1];
    RNB_TRY(launch_up_sample_step(rays_o, rays_d, sb.z[cur], sdf_old, sdf_new, gidx, n_old, B, n, n_new,
                                  (float)(64 << i), nullptr, nullptr, z_next, last ? nullptr : sb.index[i & 1],
                                  last ? nullptr : sb.pts, last ? nullptr : sb.sdf[cur ^ 1], s));
    if (!last) {
      // SDF of the new points (renderer.py:185)
      Carver c2((char*)ws + sb.pb_off, ws_bytes - sb.pb_off);
      PointBufs pbn;
      carve_points(L, c2, B * n_new, PM_SDF_ONLY, &pbn);
      RNB_TRY(forward_points(L, packed, sb.pts, B * n_new, pbn, false, false, false, nullptr, s));
      sdf_old = sb.sdf[cur ^ 1];       // this step's input row in sorted order (n entries)
      sdf_new = pbn.sdf;
      gidx = sb.index[i & 1];
      n_old = n;
    }
    cur ^= 1;
    n += n_new;
  }
  return RNB_OK;
}

// ---------------------------------------------------------------------------------------------------
// fine pass
// ---------------------------------------------------------------------------------------------------
struct RenderBufs {
  float* pts;
  float* dists;
  float* gerr_part;
  float* gerr_den;
  float* invs_part;
  PointBufs pb;
  // RNB_FLAG_INPUT_GRADS: the composite backward's per-ray / per-sample parts of the input adjoints (else nullptr)
  float* ig_cos_d;    // [B,3]
  float* ig_light;    // [kMaxRenderLights,B,3]
  float* ig_bg;       // [B,3]
  float* ig_dists;    // [B,S]
};

static int render_mode_of(int flags, const Layout& L) {
  int mode = PM_WITH_NORMAL;
  const bool use_color = !((flags & RNB_MODE_MVPS) && (flags & RNB_FLAG_NO_ALBEDO));
  if (use_color) mode |= PM_WITH_COLOR;
  if (!(flags & RNB_FLAG_FORWARD_ONLY)) mode |= PM_WITH_BACKWARD;
  (void)L;
  return mode;
}

static void carve_render(const Layout& L, Carver& c, int64_t B, int S, int flags, RenderBufs* rb) {
  rb->pts = c.take<float>(B * S * 3);
  rb->dists = c.take<float>(B * S);
  rb->gerr_part = c.take<float>(B * 2);
  rb->gerr_den = c.take<float>(1);
  rb->invs_part = c.take<float>(B);
  carve_points(L, c, B * S, render_mode_of(flags, L), &rb->pb);
  if (!(render_mode_of(flags, L) & PM_WITH_COLOR)) rb->pb.alb = c.take<float>(rb->pb.Mp * 4);
  rb->ig_cos_d = rb->ig_light = rb->ig_bg = rb->ig_dists = nullptr;
  if (flags & RNB_FLAG_INPUT_GRADS) {   // behind everything else: the rest of the layout is the one without the flag
    rb->ig_cos_d = c.take<float>(B * 3);
    rb->ig_light = c.take<float>((int64_t)kMaxRenderLights * B * 3);
    rb->ig_bg = c.take<float>(B * 3);
    rb->ig_dists = c.take<float>(B * S);
  }
}

static int check_input_grads_flag(const Layout& L, int flags) {
  if ((flags & RNB_FLAG_INPUT_GRADS) && is_bf16(L))
    RNB_FAIL(RNB_E_INVALID, "RNB_FLAG_INPUT_GRADS: RNB_VARIANT_BF16 has no input adjoints (the fp32 variants only)");
  return RNB_OK;
}

RNB_API int rnb_render_workspace_bytes(const rnb_model_desc* desc, int64_t B, int32_t S, int32_t flags,
                                       int64_t* bytes) {
  RNB_REQUIRE(bytes, "bytes");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  if (B < 0 || S < 1) RNB_FAIL(RNB_E_INVALID, "bad B/S");
  if (S > kMaxS) RNB_FAIL(RNB_E_INVALID, "samples per ray %d > %d (kMaxS)", S, kMaxS);
  RNB_TRY(check_input_grads_flag(L, flags));
  Carver c(nullptr, 0);
  RenderBufs rb;
  carve_render(L, c, B, S, flags, &rb);
  *bytes = (int64_t)c.off;
  return RNB_OK;
}

static int render_setup(const rnb_model_desc* desc, const rnb_render_args* a, void* ws, size_t ws_bytes, Layout* L,
                        RenderBufs* rb) {
  RNB_TRY(make_layout(desc, L));
  RNB_REQUIRE(a, "args");
  RNB_REQUIRE(ws, "workspace");
  if (a->B <= 0 || a->S < 1) RNB_FAIL(RNB_E_INVALID, "bad B/S");
  // the composite kernels' limits (launch_composite_fwd checks them again): refused before carve_render and any launch
  if (a->S > kMaxS) RNB_FAIL(RNB_E_INVALID, "samples per ray %d > %d (kMaxS)", a->S, kMaxS);
  const bool mvps = (a->flags & RNB_MODE_MVPS) != 0;
  if (mvps && (a->n_lights < 1 || !a->lights_dir)) RNB_FAIL(RNB_E_INVALID, "MVPS mode needs lights");
  if (mvps && a->n_lights > kMaxRenderLights)
    RNB_FAIL(RNB_E_INVALID, "n_lights %d > %d (kMaxRenderLights)", a->n_lights, kMaxRenderLights);
  if (L->F <= 0) RNB_FAIL(RNB_E_INVALID, "model has no feature head");
  RNB_REQUIRE(a->rays_o, "rays_o");
  RNB_REQUIRE(a->rays_d, "rays_d");
  RNB_REQUIRE(a->z_vals, "z_vals");
  RNB_REQUIRE(a->variance, "variance");
  RNB_TRY(check_input_grads_flag(*L, a->flags));
  Carver c(ws, ws_bytes);
  carve_render(*L, c, a->B, a->S, a->flags, rb);
  if (!c.ok) RNB_FAIL(RNB_E_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
  return RNB_OK;
}

static CompArgs comp_args_of(const Layout& L, const rnb_render_args* a, const RenderBufs& rb) {
  CompArgs c;
  memset(&c, 0, sizeof(c));
  c.B = a->B;
  c.S = a->S;
  c.L = (a->flags & RNB_MODE_MVPS) ? a->n_lights : 1;
  c.C = L.Co;
  c.flags = a->flags;
  c.cos_anneal = a->cos_anneal_ratio;
  c.rays_d = a->rays_d;
  c.pts = rb.pts;
  c.dists = rb.dists;
  c.sdf = rb.pb.sdf;
  c.nrm = rb.pb.nrm;
  c.alb = rb.pb.alb;
  c.lights = a->lights_dir;
  c.bg = (a->flags & RNB_MODE_MVPS) ? nullptr : a->background_rgb;
  c.variance = a->variance;
  c.color_fine = a->color_fine;
  c.weights = a->weights;
  c.cdf = a->cdf_fine;
  c.gradients = a->gradients;
  c.inside = a->inside_sphere;
  c.weight_sum = a->weight_sum;
  c.weight_max = a->weight_max;
  c.s_val = a->s_val;
  c.gerr_part = rb.gerr_part;
  c.sdf_out = a->sdf;
  c.albedo_out = (render_mode_of(a->flags, L) & PM_WITH_COLOR) ? a->sampled_albedo : nullptr;
  return c;
}

RNB_API int rnb_render_fwd(const rnb_model_desc* desc, const float* packed, const rnb_render_args* a, void* ws,
                           size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  RenderBufs rb;
  RNB_TRY(render_setup(desc, a, ws, ws_bytes, &L, &rb));
  RNB_REQUIRE(a->color_fine, "color_fine");
  RNB_REQUIRE(a->weights, "weights");
  RNB_REQUIRE(a->cdf_fine, "cdf_fine");
  RNB_REQUIRE(a->gradients, "gradients");
  RNB_REQUIRE(a->inside_sphere, "inside_sphere");
  RNB_REQUIRE(a->weight_sum, "weight_sum");
  RNB_REQUIRE(a->weight_max, "weight_max");
  RNB_REQUIRE(a->s_val, "s_val");
  RNB_REQUIRE(a->gradient_error, "gradient_error");
  const int mode = render_mode_of(a->flags, L);
  const bool use_color = (mode & PM_WITH_COLOR) != 0;
  RNB_TRY(launch_fine_points(a->rays_o, a->rays_d, a->z_vals, a->B, a->S, 2.0f / (float)desc->n_samples, rb.pts,
                             rb.dists, rb.pb.smax, s));
  RNB_TRY(forward_points(L, packed, rb.pts, a->B * a->S, rb.pb, true, use_color, true, nullptr, s));
  RNB_TRY(reverse_points(L, packed, rb.pb, (a->flags & RNB_FLAG_INPUT_GRADS) != 0, s));
  if (use_color) RNB_TRY(color_points(L, packed, rb.pb, rb.pts, s));
  CompArgs c = comp_args_of(L, a, rb);
  c.gerr = a->gradient_error;
  c.gerr_den = rb.gerr_den;
  c.gerr_partial = a->gerr_partial;
  RNB_TRY(launch_composite_fwd(c, s));
  return RNB_OK;
}

// Whole-image rendering: rnb_render_fwd's launches up to the composite, then the per-ray maps (composite_maps_kernel).
RNB_API int rnb_render_maps(const rnb_model_desc* desc, const float* packed, const rnb_render_args* a,
                            const rnb_render_maps_out* m, void* ws, size_t ws_bytes, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(a, "args");
  RNB_REQUIRE(m, "maps");
  hipStream_t s = (hipStream_t)stream;
  if (a->flags & RNB_FLAG_INPUT_GRADS)
    RNB_FAIL(RNB_E_INVALID, "rnb_render_maps is forward-only: RNB_FLAG_INPUT_GRADS has no meaning here");
  if (!(m->color || m->normal || m->albedo || m->depth || m->weight_sum || m->weight_max))
    RNB_FAIL(RNB_E_INVALID, "rnb_render_maps: no map requested (every output pointer is NULL)");
  rnb_render_args fa = *a;
  fa.flags |= RNB_FLAG_FORWARD_ONLY;   // the workspace of rnb_render_workspace_bytes(..., flags | RNB_FLAG_FORWARD_ONLY)
  Layout L;
  RenderBufs rb;
  RNB_TRY(render_setup(desc, &fa, ws, ws_bytes, &L, &rb));
  const int mode = render_mode_of(fa.flags, L);
  const bool use_color = (mode & PM_WITH_COLOR) != 0;
  if (m->albedo && !((fa.flags & RNB_MODE_MVPS) && use_color))
    RNB_FAIL(RNB_E_INVALID, "rnb_render_maps: the albedo map needs RNB_MODE_MVPS with the albedo network "
                            "(not RNB_MODE_CORE, not RNB_FLAG_NO_ALBEDO)");
  RNB_TRY(launch_fine_points(fa.rays_o, fa.rays_d, fa.z_vals, fa.B, fa.S, 2.0f / (float)desc->n_samples, rb.pts,
                             rb.dists, rb.pb.smax, s));
  RNB_TRY(forward_points(L, packed, rb.pts, fa.B * fa.S, rb.pb, true, use_color, true, nullptr, s));
  RNB_TRY(reverse_points(L, packed, rb.pb, false, s));
  if (use_color) RNB_TRY(color_points(L, packed, rb.pb, rb.pts, s));
  CompMapsArgs g;
  memset(&g, 0, sizeof(g));
  g.f = comp_args_of(L, &fa, rb);
  // of CompArgs' outputs the maps kernel writes these three; the per-sample pointers of `a` are ignored
  g.f.weights = g.f.cdf = g.f.gradients = g.f.inside = g.f.s_val = g.f.gerr_part = g.f.sdf_out = g.f.albedo_out = nullptr;
  g.f.color_fine = m->color;
  g.f.weight_sum = m->weight_sum;
  g.f.weight_max = m->weight_max;
  g.z = fa.z_vals;
  g.normal = m->normal;
  g.albedo = m->albedo;
  g.depth = m->depth;
  RNB_TRY(launch_composite_maps(g, s));
  return RNB_OK;
}

// rnb_render_bwd (ig == nullptr) and rnb_render_bwd_inputs
static int render_bwd_body(const rnb_model_desc* desc, const float* packed, const rnb_render_args* a,
                           const rnb_render_grads* gout, const rnb_render_input_grads* ig, float* packed_grad,
                           float* variance_grad, void* ws, size_t ws_bytes, hipStream_t s) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(gout, "gout");
  RNB_REQUIRE(packed_grad, "packed_grad");
  RNB_REQUIRE(variance_grad, "variance_grad");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  if (ig != nullptr && !(ig->rays_o || ig->rays_d || ig->lights_dir || ig->background_rgb || ig->z_vals)) ig = nullptr;
  if (ig != nullptr) {
    RNB_REQUIRE(a, "args");
    const bool mvps = (a->flags & RNB_MODE_MVPS) != 0;
    if (is_bf16(L)) RNB_FAIL(RNB_E_INVALID, "input gradients: RNB_VARIANT_BF16 has no input adjoints (the fp32 variants only)");
    if (!(a->flags & RNB_FLAG_INPUT_GRADS))
      RNB_FAIL(RNB_E_INVALID, "input gradients need a forward made with RNB_FLAG_INPUT_GRADS (it keeps their state)");
    if (ig->lights_dir && !mvps) RNB_FAIL(RNB_E_INVALID, "input gradients: lights_dir in RNB_MODE_CORE (no lights)");
    if (ig->background_rgb && (mvps || !a->background_rgb))
      RNB_FAIL(RNB_E_INVALID, "input gradients: background_rgb needs RNB_MODE_CORE with a background");
  }
  RenderBufs rb;
  RNB_TRY(render_setup(desc, a, ws, ws_bytes, &L, &rb));
  if (a->flags & RNB_FLAG_FORWARD_ONLY) RNB_FAIL(RNB_E_INVALID, "forward-only render has no backward state");
  const int mode = render_mode_of(a->flags, L);
  const bool use_color = (mode & PM_WITH_COLOR) != 0;
  // the point adjoint pbar feeds rays_o, rays_d and z; lights and background come from the composite alone
  const bool need_pbar = ig != nullptr && (ig->rays_o || ig->rays_d || ig->z_vals);
  const bool shared_lights = !(a->flags & RNB_FLAG_LIGHT_PER_RAY);
  CompBwdArgs g;
  memset(&g, 0, sizeof(g));
  g.f = comp_args_of(L, a, rb);
  g.weights = a->weights;
  g.g_color = gout->color_fine;
  g.g_weights = gout->weights;
  g.g_cdf = gout->cdf_fine;
  g.g_gradients = gout->gradients;
  g.g_weight_sum = gout->weight_sum;
  g.g_weight_max = gout->weight_max;
  g.g_s_val = gout->s_val;
  g.g_gerr = gout->gradient_error;
  g.gerr_den = rb.gerr_den;
  g.gerr_den_global = a->gerr_den_global;
  g.sbar = rb.pb.sbar;
  g.nbar = rb.pb.nbar;
  g.albbar = rb.pb.albbar;
  g.invs_part = rb.invs_part;
  g.dvar = variance_grad;
  g.amax_to_zero = rb.pb.amax;
  if (ig != nullptr) {
    g.ig_cos_d = ig->rays_d ? rb.ig_cos_d : nullptr;
    g.ig_light = ig->lights_dir ? (shared_lights ? rb.ig_light : ig->lights_dir) : nullptr;
    g.ig_bg = ig->background_rgb ? rb.ig_bg : nullptr;
    g.ig_dists = ig->z_vals ? rb.ig_dists : nullptr;
  }
  RNB_TRY(launch_composite_bwd(g, s));
  if (ig != nullptr && ig->lights_dir && shared_lights) RNB_TRY(launch_sum_over_rays(rb.ig_light, a->B, a->n_lights, ig->lights_dir, s));
  if (ig != nullptr && ig->background_rgb) RNB_TRY(launch_sum_over_rays(rb.ig_bg, a->B, 1, ig->background_rgb, s));
  RNB_CHECK_HIP(hipMemsetAsync(packed_grad, 0, (size_t)L.total * sizeof(float), s));
  if (!need_pbar) return sweep_backward(L, packed, rb.pb, use_color, packed_grad, s);
  // the render path's backward with the albedo net's encoding columns of cinb kept (color_inputs)
  RNB_TRY(sweep_backward_parts(L, packed, rb.pb, BwdParts::render(use_color, use_color), packed_grad, s));
  float* ebar = nullptr;
  RNB_TRY(launch_sdf_ebar(L, packed, rb.pb, &ebar, s));
  RayAdjArgs r;
  memset(&r, 0, sizeof(r));
  r.ebar = ebar;
  r.B = a->B;
  r.S = a->S;
  r.pts = rb.pts;
  r.dists = rb.dists;
  r.z = a->z_vals;
  r.rays_d = a->rays_d;
  r.x4 = rb.pb.x;
  r.ge = rb.pb.ge;
  r.nbar = rb.pb.nbar;
  r.nrm = rb.pb.nrm;
  r.cinb = use_color ? rb.pb.cinb : nullptr;
  r.Ep = L.Ep;
  r.multires = L.multires;
  r.Cinp = L.Cinp;
  r.F = L.F;
  r.pev = L.pev;
  r.multires_view = L.multires_view;
  r.scale = L.sdf_scale;
  r.cos_d = ig->rays_d ? rb.ig_cos_d : nullptr;
  r.dists_bar = ig->z_vals ? rb.ig_dists : nullptr;
  r.o_bar = ig->rays_o;
  r.d_bar = ig->rays_d;
  r.z_bar = ig->z_vals;
  return launch_ray_input_adjoint(r, s);
}

RNB_API int rnb_render_bwd(const rnb_model_desc* desc, const float* packed, const rnb_render_args* a,
                           const rnb_render_grads* gout, float* packed_grad, float* variance_grad, void* ws,
                           size_t ws_bytes, rnb_stream_t stream) {
  return render_bwd_body(desc, packed, a, gout, nullptr, packed_grad, variance_grad, ws, ws_bytes, (hipStream_t)stream);
}

RNB_API int rnb_render_bwd_inputs(const rnb_model_desc* desc, const float* packed, const rnb_render_args* a,
                                  const rnb_render_grads* gout, const rnb_render_input_grads* igrads, float* packed_grad,
                                  float* variance_grad, void* ws, size_t ws_bytes, rnb_stream_t stream) {
  return render_bwd_body(desc, packed, a, gout, igrads, packed_grad, variance_grad, ws, ws_bytes, (hipStream_t)stream);
}

RNB_API int rnb_render_range(const rnb_model_desc* desc, const float* packed, const void* ws, size_t ws_bytes, int64_t B, int32_t S,
                             int32_t flags, float* out, rnb_stream_t stream) {
  RNB_REQUIRE(packed, "packed");
  RNB_REQUIRE(ws, "workspace");
  RNB_REQUIRE(out, "out");
  if (B <= 0 || S < 1) RNB_FAIL(RNB_E_INVALID, "bad B/S");
  hipStream_t s = (hipStream_t)stream;
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  Carver c(const_cast<void*>(ws), ws_bytes);
  RenderBufs rb;
  carve_render(L, c, B, S, flags, &rb);
  if (!c.ok) RNB_FAIL(RNB_E_WORKSPACE, "workspace too small: need %zu bytes, have %zu", c.off, ws_bytes);
  return launch_range_report(L, packed, rb.pb, (render_mode_of(flags, L) & PM_WITH_COLOR) != 0,
                             !(flags & RNB_FLAG_FORWARD_ONLY), out, s);
}

RNB_API int rnb_profile_enable(int on) { return profile_enable(on); }
RNB_API int rnb_profile_collect(double* gemm_ms, int64_t* gemm_launches, double* gemm_flops) {
  return profile_collect(gemm_ms, gemm_launches, gemm_flops);
}
RNB_API int64_t rnb_profile_report(char* out, int64_t capacity) { return profile_report(out, capacity); }

RNB_API int rnb_algorithmic_bytes(const rnb_model_desc* desc, int64_t B, int32_t flags, double* train_bytes) {
  RNB_REQUIRE(train_bytes, "train_bytes");
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  const bool use_color = !((flags & RNB_MODE_MVPS) && (flags & RNB_FLAG_NO_ALBEDO));
  const double e = is_bf16(L) ? 2.0 : 4.0;
  const int S = desc->n_samples + desc->n_importance;
  // SDF sweeps: a, D, gz, u, zR, zb written once; D read by R, RA, FB; gz by RA, dW; zR by FB; u, zb, a by dW
  double per_pt = 15.0 * L.nh * L.Hp * e;
  per_pt += 2.0 * L.Ep * e * 2.0;   // e and u_0: written once, read once (layer 0's weight gradient)
  if (use_color) {
    // albedo network: cin (1 write, 2 reads), ac_l (1 write; read by the next layer, the relu mask and a dW), zc_l
    // (1 write, 2 reads), cinb (1 write; read by FB and by the normal's adjoint).  bf16 too when the bf16 albedo
    // kernels apply (RNB_VARIANT_BF16 with the shipped shape), else fp32.
    const double ec = L.route.color == COLOR_BF16 ? 2.0 : 4.0;
    per_pt += ec * (3.0 * L.Cinp + 4.0 * L.Hcp + 3.0 * L.Hcp * (L.nc - 1) + 3.0 * L.Hcp * L.nc + 2.0 * L.Cinp);
    per_pt += e * 2.0 * L.Hp;         // feature head's weight gradient: fbar and a_last
  }
  *train_bytes = per_pt * (double)B * S;
  return RNB_OK;
}

// Algorithmic MLP FLOPs: multiply-accumulate counts of the real (unpadded) layer shapes.
RNB_API int rnb_algorithmic_flops(const rnb_model_desc* desc, int64_t B, int32_t flags, double* train_flops,
                                  double* forward_flops) {
  Layout L;
  RNB_TRY(make_layout(desc, &L));
  double mac_s = 0;   // one SDF forward
  for (int l = 0; l < L.nh; ++l) mac_s += (double)L.hid[l].N * L.hid[l].K;
  mac_s += (double)(L.F + 1) * L.H;
  double mac_c = 0;
  for (int l = 0; l < L.nc; ++l) mac_c += (double)L.col[l].N * L.col[l].K;
  mac_c += (double)L.colo.N * L.colo.K;
  const bool use_color = !((flags & RNB_MODE_MVPS) && (flags & RNB_FLAG_NO_ALBEDO));
  const double Fs = 2.0 * mac_s, Fc = 2.0 * mac_c;
  const int S = desc->n_samples + desc->n_importance;
  const int n_new = desc->n_importance > 0 ? desc->n_importance / desc->up_sample_steps : 0;
  const double coarse_pts = desc->n_importance > 0 ? desc->n_samples + (double)n_new * (desc->up_sample_steps - 1) : 0;
  const double per_ray_train = coarse_pts * Fs + S * 6.0 * Fs + (use_color ? S * 3.0 * Fc : 0.0);
  const double per_ray_fwd = coarse_pts * Fs + S * 2.0 * Fs + (use_color ? S * Fc : 0.0);
  if (train_flops) *train_flops = per_ray_train * (double)B;
  if (forward_flops) *forward_flops = per_ray_fwd * (double)B;
  return RNB_OK;
}
