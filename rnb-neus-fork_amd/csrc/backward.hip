// The explicit backward of both networks for every route, given pb.sbar, pb.nbar, pb.albbar (from the composite backward or
// a point-wise autograd call): a list of stages, each dispatched on Layout::route to the route's own kernels (layers.hip,
// fused_bwd.hip, color_h2.hip, bf16_sweeps.hip, bf16_color.hip), then the weight-gradient jobs (dw.hip; bf16_dw.hip).  The
// point-wise kernels here are the ones more than one route launches; the input adjoints of the point-wise autograd calls
// follow.
#include "gemm.hip.h"
#include "pe.hip.h"
#include "rnb_internal.h"

namespace rnb {

// nbar_total = nbar + J_pe(n)^T cinb[pe(n) block] ;  geb = J_pe(x) nbar_total  (input of the RA sweep)
// One wave = 64 points.  The [pe(p) | pe(n)] block of cinb (columns blk_off .. Cinp) comes in through an LDS
// tile, the geb rows go out through one; dynamic LDS = 64 * (max(Cinp - blk_off, Ep) + 1) floats.
__global__ __launch_bounds__(64) void nbar_geb_kernel(const float* __restrict__ x4, const float* __restrict__ nrm,
                                                      const float* __restrict__ nbar_in,
                                                      const float* __restrict__ cinb, int Cinp, int blk_off,
                                                      int pen_off, int multires_view, int with_color, int multires,
                                                      int Ep, int64_t M, int64_t Mp, float* __restrict__ geb,
                                                      unsigned* __restrict__ amax) {
  extern __shared__ float tile[];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64, row = r0 + lane;
  float nb[3] = {0.f, 0.f, 0.f};
  if (with_color) {
    const int Wc = Cinp - blk_off;
    tile_load64(cinb, Cinp, r0, blk_off, Wc, tile, lane);
    __builtin_amdgcn_wave_barrier();
    if (row < M) {
      const float* g = tile + lane * (Wc + 1) + (pen_off - blk_off);
#pragma unroll
      for (int d = 0; d < 3; ++d) nb[d] = nbar_in[row * 4 + d] + g[d];
      pe_adjoint(nrm + row * 4, g, multires_view, 0, 1, nb);
    }
    __builtin_amdgcn_wave_barrier();   // every lane is done with the input tile before it is overwritten
  } else if (row < M) {
#pragma unroll
    for (int d = 0; d < 3; ++d) nb[d] = nbar_in[row * 4 + d];
  }
  float* o = tile + lane * (Ep + 1);
  o[0] = nb[0]; o[1] = nb[1]; o[2] = nb[2];
  float gm = fmaxf(fmaxf(fabsf(nb[0]), fabsf(nb[1])), fabsf(nb[2]));   // max |geb| of this row (rows >= M carry nb = 0)
  pe_tangent(x4 + row * 4, nb, multires, 0, 1, [&](int c, float v0, float v1) {
    o[c] = v0;
    o[c + 3] = v1;
    gm = fmaxf(gm, fmaxf(fabsf(v0), fabsf(v1)));
  });
  for (int c = 3 + 6 * multires; c < Ep; ++c) o[c] = 0.f;
  if (amax != nullptr) amax_commit(amax, gm, lane);   // the scale of layer 0's weight-gradient job (x2h)
  __builtin_amdgcn_wave_barrier();
  tile_store64(geb, Ep, r0, 0, Ep, tile, lane);
}

// gradient of the sdf-head row: dw_sdf[k] += sum_rows ( sbar/scale * a_last + u_last ), db_sdf += sum sbar/scale
// A workgroup owns 32 columns (blockIdx.y) and a slab of rows (blockIdx.x): thread = (4 columns, one of 64 row
// phases), i.e. every row contributes one 128-byte line per matrix, and an output address only receives one
// atomic per row slab (same-address atomics serialise in the L2: with whole-row workgroups every address took
// one atomic from every workgroup).  fp64 partial sums (long signed sums).
// ulast == nullptr: u_nh arrives as per-tile column sums `ucol` [ntiles][Hp] (fused RA sweep), added by the first row slab.
__global__ __launch_bounds__(512) void sdf_head_bwd_kernel(const float* __restrict__ a, const float* __restrict__ ulast,
                                                           const float* __restrict__ ucol, int ntiles,
                                                           int Hp, int H, const float* __restrict__ sbar,
                                                           float inv_scale, int64_t M, int rows_per_blk,
                                                           float* __restrict__ dwsdf, float* __restrict__ dbsdf,
                                                           float* __restrict__ part_w, float* __restrict__ part_b) {
  // part_w != nullptr: this row slab's sums go to part_w[slab][Hp] / part_b[slab] with plain stores (summed in slab order by
  // dw_reduce_kernel: bit-reproducible) instead of into dwsdf / dbsdf through fp32 atomics
  __shared__ double red[64][33];
  __shared__ double redb[64];
  const int tid = threadIdx.x, cg = tid & 7, ph = tid >> 3;
  const int kl = cg * 4, k0 = blockIdx.y * 32 + kl;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk;
  const int64_t r1 = min(M, r0 + rows_per_blk);
  double s[4] = {0.0, 0.0, 0.0, 0.0}, sb = 0.0;
#pragma unroll 4
  for (int64_t row = r0 + ph; row < r1; row += 64) {
    const float t = sbar[row] * inv_scale;
    if (cg == 0) sb += (double)t;
    const vf4 av = *reinterpret_cast<const vf4*>(a + row * Hp + k0);
    if (ulast != nullptr) {
      const vf4 uv = *reinterpret_cast<const vf4*>(ulast + row * Hp + k0);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += (double)(t * av[j] + uv[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += (double)(t * av[j]);
    }
  }
  if (ulast == nullptr && blockIdx.x == 0) {
    for (int tile = ph; tile < ntiles; tile += 64) {
      const vf4 uv = *reinterpret_cast<const vf4*>(ucol + (size_t)tile * Hp + k0);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += (double)uv[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[ph][kl + j] = s[j];
  if (cg == 0) redb[ph] = sb;
  __syncthreads();
  if (tid < 32) {
    double t = 0.0;
    for (int q = 0; q < 64; ++q) t += red[q][tid];
    const int col = blockIdx.y * 32 + tid;
    if (part_w != nullptr) part_w[(size_t)blockIdx.x * Hp + col] = col < H ? (float)t : 0.f;
    else if (col < H) atomicAdd(dwsdf + col, (float)t);
  } else if (tid == 32 && blockIdx.y == 0) {
    double t = 0.0;
    for (int q = 0; q < 64; ++q) t += redb[q];
    if (part_b != nullptr) part_b[blockIdx.x] = (float)t;
    else atomicAdd(dbsdf, (float)t);
  }
}

// ---- input adjoints of the point-wise autograd calls (rnb_sdf_backward / rnb_color_backward) ----------------------
// x's adjoint of the SDF network (models/fields.py:84, :104, :114-127 under autograd):
//   xbar = scale * ( J_pe(xs)^T ebar + [normal] sum_k ge_k d^2 pe_k / d xs^2 . nbar ),   xs = scale * x,
// ebar = d loss / d e (FB's zb_0 W_0 plus the skip layer's encoding columns, launch_sdf_ebar).  The second term is diagonal
// per coordinate: d^2 sin(f x) = -f^2 sin(f x), d^2 cos(f x) = -f^2 cos(f x), f = 2^k; ge = d sdf / d e from the R sweep.
__global__ void sdf_xbar_kernel(const float* __restrict__ x4, const float* __restrict__ ebar, const float* __restrict__ ge,
                                const float* __restrict__ nbar, int Ep, int multires, float scale, int64_t M,
                                float* __restrict__ xbar) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= M) return;
  const float* eb = ebar + row * Ep;
  float acc[3] = {eb[0], eb[1], eb[2]};
  const float* g = ge != nullptr ? ge + row * Ep : nullptr;
  pe_adjoint_hess(x4 + row * 4, eb, g != nullptr, g, nbar + row * 4, multires, 0, 1, acc);
#pragma unroll
  for (int d = 0; d < 3; ++d) xbar[row * 3 + d] = scale * acc[d];
}

// adjoints of the albedo net's encoded inputs: pbar = J_pe(p)^T cinb[pe(p)], nbar = J_pe(n)^T cinb[pe(n)] (either may be
// NULL).  p, n: the saved inputs [Mp,4]; cinb complete (the per-layer backward, or color_h2 with keep_pe).
__global__ void color_input_bwd_kernel(const float* __restrict__ cinb, int Cinp, int F, int pev, int multires_view,
                                       const float* __restrict__ p4, const float* __restrict__ n4, int64_t M,
                                       float* __restrict__ pbar, float* __restrict__ nbar) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= M) return;
  for (int which = 0; which < 2; ++which) {
    float* out = which ? nbar : pbar;
    if (out == nullptr) continue;
    const float* g = cinb + row * Cinp + F + which * pev;
    const float* v = (which ? n4 : p4) + row * 4;
    float t[3] = {g[0], g[1], g[2]};
    pe_adjoint(v, g, multires_view, 0, 1, t);
#pragma unroll
    for (int d = 0; d < 3; ++d) out[row * 3 + d] = t[d];
  }
}

// ---- the stages that are the same launch on more than one route ----------------------------------------------------

// nbar (+ the albedo net's contribution through cinb) -> geb = u_0, the input of the RA sweep
static int launch_nbar_geb(const Layout& L, PointBufs& pb, bool with_color, hipStream_t s) {
  const int wt = (with_color && L.Cinp - L.F > L.Ep) ? L.Cinp - L.F : L.Ep;
  hipLaunchKernelGGL(nbar_geb_kernel, dim3(blocks_for(pb.Mp, 64)), dim3(64), (size_t)64 * (wt + 1) * sizeof(float), s,
                     pb.x, pb.nrm, pb.nbar, pb.cinb, L.Cinp, L.F, L.F + L.pev, L.multires_view, with_color ? 1 : 0,
                     L.multires, L.Ep, pb.M, pb.Mp, pb.geb, (unsigned*)nullptr);   // (max |geb|: recorded by the RA sweep as it loads the tile)
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// gradient of the sdf-head row.  u_rows: u_nh arrives as rows (per-layer RA), else as `u_tiles` per-tile column sums
// (fused RA; 0 without the normal).  *slabs_out: the number of slabs left in pb.sdfh_part for dw_backward, or 0.
static int launch_sdf_head_bwd(const Layout& L, PointBufs& pb, bool u_rows, int u_tiles, float* packed_grad, int* slabs_out,
                               hipStream_t s) {
  const int64_t M = pb.M;
  // Hp / 32 column chunks x row slabs, ~256 workgroups in total, slabs a multiple of the 64 row phases
  const int chunks = L.Hp / 32;
  int64_t slabs = (L.variant & RNB_VARIANT_DETERMINISTIC) ? 1 : (256 + chunks - 1) / chunks;
  // with the one-workgroup-per-gradient kernel there is a slab reduction at the end of the backward: the row slabs'
  // sums ride in it (no atomics: bit-reproducible); otherwise fp32 atomics (one slab in the deterministic variant)
  const bool slab_out = dw_one_wg_runs(L, M);
  if (slab_out) slabs = kSdfHeadSlabs;
  int rows_per_blk = (int)((M + slabs - 1) / slabs);
  rows_per_blk = (rows_per_blk + 63) / 64 * 64;
  const unsigned nslab = blocks_for(M, rows_per_blk);
  hipLaunchKernelGGL(sdf_head_bwd_kernel, dim3(nslab, chunks), dim3(512), 0, s, pb.a[L.nh - 1],
                     u_rows ? (const float*)pb.u[L.nh] : (const float*)nullptr, (const float*)pb.u[L.nh], u_tiles, L.Hp,
                     L.H, pb.sbar, 1.f / L.sdf_scale, M, rows_per_blk, packed_grad + L.wsdf_off, packed_grad + L.bsdf_off,
                     slab_out ? pb.sdfh_part : nullptr, slab_out ? pb.sdfh_part + (size_t)nslab * L.Hp : nullptr);
  RNB_CHECK_LAUNCH();
  *slabs_out = slab_out ? (int)nslab : 0;
  return RNB_OK;
}

// A route-specific buffer that the workspace mode did not carve is an error, never a reason to take another route
// (carve_points carves from the same Layout::route, so no entry point gets here).
static int check_route_buffers(const Layout& L, const PointBufs& pb, const BwdParts& parts) {
  const Route& r = L.route;
  const char* missing = nullptr;
  if (r.h2 && pb.amax == nullptr) missing = "amax";
  else if (r.h2 && pb.smax == nullptr) missing = "smax";
  else if (parts.albedo && r.color == COLOR_BF16 && pb.cin8 == nullptr) missing = "cin8";
  else if (parts.albedo && r.color == COLOR_H2 && pb.col_part == nullptr) missing = "col_part";
  else if (parts.sdf && r.sdf != SDF_BF16 && dw_one_wg_runs(L, pb.M) && pb.sdfh_part == nullptr) missing = "sdfh_part";
  if (missing != nullptr) RNB_FAIL(RNB_E_WORKSPACE, "backward: this workspace has no PointBufs::%s, which the model's kernel route needs", missing);
  return RNB_OK;
}

// ---- the backward --------------------------------------------------------------------------------------------------

// A render's backward.  packed_grad (same layout as `packed`) must be zero on entry; it receives dW_eff / db of every layer.
int sweep_backward(const Layout& L, const float* packed, PointBufs& pb, bool with_color, float* packed_grad, hipStream_t s) {
  return sweep_backward_parts(L, packed, pb, BwdParts::render(with_color, false), packed_grad, s);
}

// The backward in parts (a render; point-wise autograd of the direct network calls, api.hip):
//   albedo        C' from pb.albbar: the albedo net's weight gradients and cinb
//   sdf           the SDF half: sdf-head row, FB, dW of every hidden layer (seeded by pb.sbar)
//   feat          FB's feature-head seed is cinb's feature block (the albedo backward's, or a caller-supplied adjoint)
//   normal        pb.nbar is live: nbar -> geb, the RA sweep and the gz/u weight-gradient pairs.  Without it RA is skipped,
//                 zR_l is zero and the layers' weight gradients are the single zb/a pair
//   color_inputs  cinb is left complete, encoding columns included, for the input adjoints
// (pb.amax was zeroed by the composite backward, the first kernel of rnb_render_bwd, or by the point-wise entry point.)
// The zero-tile path (color_h2.hip): on in a render's backward of the fused fp32 route whose FB sweep skips
// the tile too (fused_fb_h2_kernel) and where no caller waits for cinb's encoding columns (color_inputs: the tile's word lies
// there).  Where the weight-gradient jobs skip the tile too (gemm_dw_x3_kernel: BwdParts::dead_dw) its rows of zc_l and cinb
// stay unwritten; elsewhere (a point count that is no multiple of 32 goes to the split-K kernels) the dead tile stores zeros.
bool dead_tiles_on(const Layout& L, const PointBufs& pb, const BwdParts& parts) {
  return !(L.variant & RNB_VARIANT_NO_DEAD_TILES) && parts.albedo && parts.sdf && !parts.color_inputs && L.route.color == COLOR_H2 &&
         L.route.h2 && pb.alb_dead != nullptr && pb.smax != nullptr && fused_fb_honours_dead(L);
}

int sweep_backward_parts(const Layout& L, const float* packed, PointBufs& pb, const BwdParts& parts_in, float* packed_grad,
                         hipStream_t s) {
  const Route& r = L.route;
  BwdParts parts = parts_in;
  parts.dead_tiles = dead_tiles_on(L, pb, parts_in);
  parts.dead_dw = parts.dead_tiles && dw_honours_dead(L, pb.M);
  RNB_TRY(check_route_buffers(L, pb, parts));
  RNB_TRY(dw_zero_partials(L, pb, s));
  // the weight-gradient jobs (dw.hip) follow every other launch of the backward; bf16_color_backward's are bf16_dw_backward's
  BwdParts dw_parts = parts;
  dw_parts.albedo = parts.albedo && r.color != COLOR_BF16;
  // ---- C': albedo network backward ---------------------------------------------------------------
  // (color_h2_backward is ONE fused sweep, which with parts.sdf also forms geb = J_pe(x) nbar_total)
  if (parts.albedo) switch (r.color) {
    case COLOR_BF16: RNB_TRY(bf16_color_backward(L, packed, pb, packed_grad, s)); break;
    case COLOR_H2: RNB_TRY(color_h2_backward(L, packed, pb, s, parts.sdf, parts.color_inputs, parts.dead_tiles, !parts.dead_dw)); break;
    case COLOR_LAYERS: RNB_TRY(layers_color_backward(L, packed, pb, packed_grad, s)); break;
    case COLOR_NONE: RNB_FAIL(RNB_E_INVALID, "backward: the model has no albedo network");
  }
  if (!parts.sdf) return dw_backward(L, pb, dw_parts, 0, packed_grad, s);
  // ---- nbar (+ albedo-net contribution) -> geb = u_0 -----------------------------------------------
  if (parts.normal && !(parts.albedo && r.color == COLOR_H2)) RNB_TRY(launch_nbar_geb(L, pb, parts.albedo, s));
  const bool bf = r.sdf == SDF_BF16;   // (the render path only: every part is on, api.hip refuses the point-wise calls)
  if (bf) {
    // The albedo net's fp32 weight-gradient jobs (fp32 albedo kernels behind bf16 SDF sweeps) run HERE, before RA, not at
    // the end: bf16_dw_backward reuses pb.dw_part from its base and, in the deterministic variant, zeroes all of it and
    // fills it with its own slabs.  The fp32 split-K kernels ACCUMULATE into slabs that dw_zero_partials zeroed above; run
    // after the bf16 jobs they would add onto dirty slabs.
    dw_parts.sdf = false;
    RNB_TRY(dw_backward(L, pb, dw_parts, 0, packed_grad, s));
  }
  // ---- RA: adjoint of the reverse sweep, forward layer order -----------------------------------------
  int u_tiles = 0;
  if (bf) {
    RNB_TRY(bf16_ra(L, packed, pb, s));
  } else if (!parts.normal) {   // nbar == 0: RA's outputs are zero; FB adds zR_l, the layers' weight gradients skip the u pairs
    for (int l = 0; l < L.nh; ++l) RNB_CHECK_HIP(hipMemsetAsync(pb.zR[l], 0, (size_t)pb.Mp * L.Hp * sizeof(float), s));
  } else if (r.sdf == SDF_FUSED) {
    RNB_TRY(fused_ra(L, packed, pb, s, &u_tiles));
  } else {
    RNB_TRY(layers_ra(L, packed, pb, s));
  }
  // ---- sdf-head row gradient ---------------------------------------------------------------------
  int sdfh_slabs = 0;
  if (bf) RNB_TRY(bf16_sdf_head_bwd(L, pb, packed_grad, s));
  else RNB_TRY(launch_sdf_head_bwd(L, pb, parts.normal && r.sdf == SDF_LAYERS, u_tiles, packed_grad, &sdfh_slabs, s));
  // ---- FB: all zb_l (one launch on the fused and bf16 routes) ----------------------------------------
  switch (r.sdf) {
    case SDF_BF16: RNB_TRY(bf16_fb(L, packed, pb, parts.albedo, s)); break;
    case SDF_FUSED: RNB_TRY(fused_fb(L, packed, pb, parts.feat, s, parts.dead_tiles)); break;
    case SDF_LAYERS: RNB_TRY(layers_fb(L, packed, pb, parts.feat, s)); break;
  }
  // ---- dW --------------------------------------------------------------------------------------------
  if (bf) return bf16_dw_backward(L, pb, parts.albedo, packed_grad, s);
  return dw_backward(L, pb, dw_parts, sdfh_slabs, packed_grad, s);
}

// ---- input adjoints of the point-wise autograd calls ---------------------------------------------------------------

// x's adjoint after an SDF backward: ebar (launch_sdf_ebar) + one point-wise kernel.  Needs pb.x and, with_normal, pb.ge
// (R sweep) and pb.nbar.
int launch_sdf_xbar(const Layout& L, const float* packed, PointBufs& pb, bool with_normal, float* xbar, hipStream_t s) {
  float* ebar = nullptr;
  RNB_TRY(launch_sdf_ebar(L, packed, pb, &ebar, s));
  hipLaunchKernelGGL(sdf_xbar_kernel, dim3(blocks_for(pb.M, 256)), dim3(256), 0, s, pb.x, ebar,
                     with_normal ? (const float*)pb.ge : nullptr, pb.nbar, L.Ep, L.multires, L.sdf_scale, pb.M, xbar);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

int launch_color_input_bwd(const Layout& L, const PointBufs& pb, float* pts_bar, float* nrm_bar, hipStream_t s) {
  if (pts_bar == nullptr && nrm_bar == nullptr) return RNB_OK;
  hipLaunchKernelGGL(color_input_bwd_kernel, dim3(blocks_for(pb.M, 256)), dim3(256), 0, s, pb.cinb, L.Cinp, L.F, L.pev,
                     L.multires_view, pb.x, pb.nrm, pb.M, pts_bar, nrm_bar);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

}  // namespace rnb
