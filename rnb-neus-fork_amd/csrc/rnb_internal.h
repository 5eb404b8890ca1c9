// Internal declarations shared by the translation units of librnbneus_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/rnbneus.h"
#include "bf16_dw_plan.h"

namespace rnb {

constexpr int kPad = 32;          // every feature width is padded to the MFMA tile width
constexpr int kRowPad = 128;      // point counts are padded to the GEMM block height
inline int pad32(int x) { return (x + kPad - 1) / kPad * kPad; }
inline int64_t pad_rows(int64_t m) { return (m + kRowPad - 1) / kRowPad * kRowPad; }
inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

void set_error(const char* fmt, ...);
#define RNB_FAIL(code, ...)        \
  do {                             \
    ::rnb::set_error(__VA_ARGS__); \
    return (code);                 \
  } while (0)
#define RNB_CHECK_HIP(expr)                                                          \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) RNB_FAIL(RNB_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define RNB_CHECK_LAUNCH() RNB_CHECK_HIP(hipGetLastError())
#define RNB_TRY(expr)          \
  do {                         \
    int rc_ = (expr);          \
    if (rc_ != RNB_OK) return rc_; \
  } while (0)

// One linear layer inside the packed (effective-weight) buffer: W [Np x Kp] row-major, then b [Np].
struct Lin {
  int N, K;        // real out / in widths
  int Np, Kp;      // padded
  int64_t w_off;   // float offset of W in the packed buffer
  int64_t wT_off;  // float offset of the transposed copy W^T [Kp x Np] (reverse-shaped sweeps), or -1
  int64_t b_off;   // float offset of b
  float scale;     // factor folded into W (1/sqrt2 for the skip layer)
};
// algorithmic FLOPs of one layer-shaped GEMM over M points: real (unpadded) layer shape
inline double mm_flops(int64_t M, const Lin& ln) { return 2.0 * (double)M * ln.N * ln.K; }

// The kernel route of each network: a function of the descriptor alone, decided once by make_layout.  Forward, backward
// and carve_points all read it, so the buffers carved, the sweeps that fill them and the backward that reads them agree.
enum SdfRoute { SDF_LAYERS, SDF_FUSED, SDF_BF16 };   // per-layer chain (layers.hip) | fused.hip / fused_bwd.hip | bf16_sweeps.hip
enum ColorRoute { COLOR_NONE, COLOR_LAYERS, COLOR_H2, COLOR_BF16 };   // no albedo net | layers.hip | color_h2.hip | bf16_color.hip
struct Route {
  SdfRoute sdf;
  ColorRoute color;
  bool h2;   // x2h weight gradients: every producer records the maximum of its tensor, the dW jobs scale by them
};

// Packed layout of both networks (see weightnorm.hip for how leaves map onto it).
struct Layout {
  // SDF network: nh hidden layers (softplus) + output layer split into sdf row and feature rows
  int nh;                 // number of hidden (softplus) layers = sdf_n_layers
  int pe;                 // positional-encoding width (39)
  int Ep;                 // padded pe width
  int H, Hp;              // hidden width, padded
  int skip;               // skip layer index or -1
  Lin hid[RNB_MAX_LIN];   // hidden layers 0..nh-1
  int F, Fp;              // feature width (d_out-1), padded
  Lin feat;               // rows 1.. of the last layer (feature head)
  int64_t wsdf_off;       // row 0 of the last layer [Hp]
  int64_t bsdf_off;       // its bias [1] (padded to 32)
  float sdf_scale;
  int multires;
  // albedo network: nc hidden (relu) layers + output layer (d_out rows, sigmoid)
  int nc;
  int pev;                // pe width of multires_view (27)
  int Cin, Cinp;          // input width (F + 2*pev), padded
  int Hc, Hcp;
  int Co, Cop;            // d_out, padded to 32
  Lin col[RNB_MAX_LIN];   // hidden layers 0..nc-1
  Lin colo;               // output layer
  int multires_view;
  int squeeze;
  int64_t total;          // floats of fp32 packed weights (also the length of a gradient buffer)
  int64_t total_all;      // floats of the packed buffer = total (+ total / 2 for the bf16 mirror, RNB_VARIANT_BF16)
  int64_t h2tab_off;      // RNB_VARIANT_X2H: float offset of the scale table of the fp16 mirror (H2Tab), else -1
  int variant;            // rnb_model_desc.variant (RNB_VARIANT_* bits)
  int knob(int shift) const { return (variant >> shift) & 3; }
  Route route;            // which kernels run the two networks (make_layout's last step)
};

int make_layout(const rnb_model_desc* d, Layout* L);

// The SDF network as its sweep kernels read it (fused.hip / fused_bwd.hip, sweep_mv.hip, bf16_sweeps.hip): the layer table of the
// Layout, by value inside every sweep's argument struct.  Offsets are float offsets into the packed buffer.
struct SdfNetArgs {
  int nh, skip, pe, multires, Ep;
  float scale, inv_scale;      // sdf_scale and its reciprocal
  int n_real[RNB_MAX_LIN];     // real output width of hidden layer l
  int Kp[RNB_MAX_LIN];         // padded input width of hidden layer l
  long long w_off[RNB_MAX_LIN], b_off[RNB_MAX_LIN], wT_off[RNB_MAX_LIN];
  long long wsdf_off, bsdf_off;
  int F, Cinp;                 // feature head: real rows, padded width of the albedo-net input it is written into
  long long wf_off, bf_off, wfT_off;
};
inline SdfNetArgs sdf_net_args(const Layout& L) {
  SdfNetArgs n;
  memset(&n, 0, sizeof(n));
  n.nh = L.nh; n.skip = L.skip; n.pe = L.pe; n.multires = L.multires; n.Ep = L.Ep;
  n.scale = L.sdf_scale;
  n.inv_scale = 1.f / L.sdf_scale;
  for (int l = 0; l < L.nh; ++l) {
    n.n_real[l] = L.hid[l].N;
    n.Kp[l] = L.hid[l].Kp;
    n.w_off[l] = L.hid[l].w_off;
    n.b_off[l] = L.hid[l].b_off;
    n.wT_off[l] = L.hid[l].wT_off;
  }
  n.wsdf_off = L.wsdf_off;
  n.bsdf_off = L.bsdf_off;
  n.F = L.F;
  n.Cinp = L.Cinp;
  n.wf_off = L.feat.w_off; n.bf_off = L.feat.b_off; n.wfT_off = L.feat.wT_off;
  return n;
}
// algorithmic FLOPs of an SDF-network sweep over M points: hidden layers first .. nh - 1, the sdf row, the feature head
inline double sdf_sweep_flops(const Layout& L, int64_t M, int first, bool sdf_row, bool feat) {
  double fl = 0;
  for (int l = first; l < L.nh; ++l) fl += mm_flops(M, L.hid[l]);
  if (sdf_row) fl += 2.0 * (double)M * L.H;
  if (feat) fl += 2.0 * (double)M * L.F * L.H;
  return fl;
}

// Run-time value -> template argument: pick_c<A, B, ...>(v, f) calls f(std::integral_constant<int, X>{}) for the listed X
// that equals v (the last one listed takes every other v).  Nested, they map a launcher's run-time choices to ONE kernel
// instantiation that is called directly: only the listed combinations are instantiated, and the launch takes its block size
// from the same constants as the kernel's __launch_bounds__.
template <int V0, int... Vs, class F>
inline void pick_c(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
  else if (v == V0) f(std::integral_constant<int, V0>{});
  else pick_c<Vs...>(v, f);
}

#if defined(__HIPCC__)
// torch.clamp / torch.minimum / torch.max / F.relu PROPAGATE NaN; fmaxf / fminf (v_max_f32 / v_min_f32) return the
// other operand.  A diverged model must come back as NaN exactly where the reference's does, so the element-wise
// min / max of the path go through these.  Identical to fminf / fmaxf on numbers.
__device__ inline float max_nan(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
__device__ inline float min_nan(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
__device__ inline float clamp_nan(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }
__device__ inline float relu_nan(float x) { return x < 0.f ? 0.f : x; }

// torch.linspace(start, end, steps)[i] as ATen's CPU kernel computes it: step = (end-start)/(steps-1); first half
// start + step*i, second half end - step*(steps-1-i), each as one fused multiply-add (explicit fmaf: independent of
// the translation unit's contraction mode).
__device__ inline float linspace_at(float start, float end, int steps, int i) {
  if (steps == 1) return start;
  const float step = (end - start) / (float)(steps - 1);
  return i < steps / 2 ? fmaf(step, (float)i, start) : fmaf(-step, (float)(steps - 1 - i), end);
}
#endif

// regular grid of extract_fields, generated inside the forward kernel (rnb_sdf_grid)
// on == GRID_BRICKS / GRID_LATTICE (rnb_sdf_grid_sparse_*, sparse_grid.hip): the rows are samples of the SAME grid, picked
// by index, so a value is the very number the dense sweep computes there.
//   GRID_BRICKS : row r -> brick bricks[r / rows_per_brick] (linear id (bx * nb + by) * nb + bz), local sample
//                 r % rows_per_brick -> (lx, ly, lz) in a (bs + 1)^3 cube, i = b * bs + l; rows past (bs + 1)^3 and samples
//                 past res - 1 (a short last brick) are masked; the value is SCATTERED to volume[(ix * res + iy) * res + iz]
//   GRID_LATTICE: row r -> brick corner (kx, ky, kz) of the (nb + 1)^3 lattice, i = min(k * bs, res - 1); value -> out[r]
enum { GRID_OFF = 0, GRID_DENSE = 1, GRID_BRICKS = 2, GRID_LATTICE = 3 };
struct GridGen {
  int on;
  int res, x_begin;
  float bmin[3], bmax[3];
  float out_scale;
  const int32_t* bricks;   // GRID_BRICKS: the brick list (device)
  int bs, nb;              // cells per brick edge, bricks per axis
  int rows_per_brick;      // (bs + 1)^3 rounded up to the 64-point tile
  int64_t family_rows;     // != 0: the launcher picks the kernel family of a sweep over this many rows (the dense grid's), so
                           // that a sparse sample carries the dense sample's bits
};
inline int64_t family_rows_of(const GridGen* g, int64_t Mp) { return g != nullptr && g->family_rows != 0 ? g->family_rows : Mp; }

#if defined(__HIPCC__)
// Grid sample of row `row` of a sweep over M rows: its indices, and where its value goes (-1: a masked row — it computes on
// the origin like a padding row and stores nothing).  GRID_DENSE is rnb_sdf_grid's arithmetic unchanged.
__device__ inline int64_t grid_locate(const GridGen& g, int64_t row, int64_t M, int& ix, int& iy, int& iz) {
  if (row >= M) return -1;
  if (g.on == GRID_DENSE) {   // row = ((ix - x_begin) * res + iy) * res + iz of the slab
    int64_t r = row;
    iz = (int)(r % g.res);
    r /= g.res;
    iy = (int)(r % g.res);
    ix = (int)(r / g.res) + g.x_begin;
    return row;
  }
  if (g.on == GRID_BRICKS) {
    const int n1 = g.bs + 1;
    const int l = (int)(row % g.rows_per_brick);
    if (l >= n1 * n1 * n1) return -1;
    int b = g.bricks[row / g.rows_per_brick];
    const int bz = b % g.nb;
    b /= g.nb;
    ix = (b / g.nb) * g.bs + l / (n1 * n1);
    iy = (b % g.nb) * g.bs + (l / n1) % n1;
    iz = bz * g.bs + l % n1;
    if (ix >= g.res || iy >= g.res || iz >= g.res) return -1;
    return ((int64_t)ix * g.res + iy) * g.res + iz;
  }
  const int nl = g.nb + 1;   // GRID_LATTICE
  int64_t r = row;
  iz = min((int)(r % nl) * g.bs, g.res - 1);
  r /= nl;
  iy = min((int)(r % nl) * g.bs, g.res - 1);
  ix = min((int)(r / nl) * g.bs, g.res - 1);
  return row;
}
// the store side of the same mapping
__device__ inline int64_t grid_out_index(const GridGen& g, int64_t row, int64_t M) {
  if (g.on == GRID_DENSE) return row < M ? row : -1;
  int ix, iy, iz;
  return grid_locate(g, row, M, ix, iy, iz);
}

// ---- the front and the tail the forward sweeps share (fused.hip, sweep_mv.hip, bf16_sweeps.hip) ----
// The scaled point of row `row` of a sweep over M rows: the grid sample of the row (grid.on: dense slab, brick list or
// brick-corner lattice) or row `row` of pts, times scale; masked and padding rows compute on the origin.
__device__ inline void sweep_point(const GridGen& grid, const float* pts, int64_t row, int64_t M, float scale, float (&x)[3]) {
  x[0] = x[1] = x[2] = 0.f;
  if (row < M) {
    if (grid.on) {
      const int res = grid.res;
      int ix, iy, iz;
      if (grid_locate(grid, row, M, ix, iy, iz) >= 0) {
        x[0] = linspace_at(grid.bmin[0], grid.bmax[0], res, ix) * scale;
        x[1] = linspace_at(grid.bmin[1], grid.bmax[1], res, iy) * scale;
        x[2] = linspace_at(grid.bmin[2], grid.bmax[2], res, iz) * scale;
      }
    } else {
      x[0] = pts[row * 3] * scale;
      x[1] = pts[row * 3 + 1] * scale;
      x[2] = pts[row * 3 + 2] * scale;
    }
  }
}
// The sdf of row row0 + r (r: the row inside the tile at row0) -> its place: sdf[row], or with a grid the sample's entry of
// the volume times out_scale (the volume has exactly M entries; brick mode scatters — a face sample shared by two listed
// bricks is written by both with the same bits: same coordinates, same kernel family, rows independent of their tile mates;
// masked rows store nothing).
__device__ inline void sweep_store_sdf(const GridGen& grid, float* sdf, int64_t row0, int r, int64_t M, float v) {
  if (!grid.on) sdf[row0 + r] = v;
  else {
    const int64_t o = grid_out_index(grid, row0 + r, M);
    if (o >= 0) sdf[o] = v * grid.out_scale;
  }
}
#endif

// ---- workspace carving ------------------------------------------------------------------------
struct Carver {
  char* base;
  size_t cap;
  size_t off = 0;
  bool ok = true;
  Carver(void* p, size_t bytes) : base((char*)p), cap(bytes) {}
  template <class T>
  T* take(int64_t n) {
    size_t bytes = ((size_t)n * sizeof(T) + 255) / 256 * 256;
    T* p = (T*)(base ? base + off : nullptr);
    off += bytes;
    if (base && off > cap) ok = false;
    return p;
  }
};

// ---- RNB_VARIANT_X2H: scales of the fp16 mirror -----------------------------------------------------------------------
// Every matrix of the fp16 mirror is stored times a power of two chosen from the matrix's own maximum: 2^8 while
// max |w| < 64 (the round-4 constant), else the power of two that puts the maximum in [2^13, 2^14) — so NO weight is out of
// range.  The table sits behind the mirror in the packed buffer (256 floats): per matrix id the float bits of max |w|
// (atomicMax by x3_pack_kernel, zeroed by wn_fwd_kernel), the scale and its inverse (written by x2h_pack_kernel, read by
// every kernel that multiplies with the mirror).  ids: hidden layer l -> l, feature head -> nh, albedo hidden layer l ->
// nh + 1 + l; W and W^T share an id.
constexpr int kH2TabSlots = 48;
struct H2Tab {
  unsigned wmax[kH2TabSlots];
  float ws[kH2TabSlots];
  float iws[kH2TabSlots];
};
static_assert(sizeof(H2Tab) <= 256 * sizeof(float), "the packed buffer reserves 256 floats for the table");
inline int h2_id_hid(int l) { return l; }

// State of one batch of points going through the SDF (+albedo) network(s).  All activation matrices
// are [Mp x width_padded] row-major fp32.
struct PointBufs {
  int64_t M, Mp;
  float* x;       // [Mp,4]   scaled points (x,y,z,0)
  float* e;       // [Mp,Ep]  positional encoding
  float* a[RNB_MAX_LIN];   // hidden activations a_l  [Mp,Hp]
  float* D[RNB_MAX_LIN];   // softplus'(z_l) = sigmoid(100 z_l)  [Mp,Hp]   (only with_normal; else nullptr)
  float* gz[RNB_MAX_LIN];  // reverse sweep state gz_l  [Mp,Hp]   (only with_normal)
  float* ge;      // [Mp,Ep]  d sdf / d e
  float* sdf;     // [Mp]
  float* nrm;     // [Mp,4]   d sdf / d x
  float* cin;     // [Mp,Cinp] albedo-net input  [feat | pe(p) | pe(n) | 0]
  float* ac[RNB_MAX_LIN];  // albedo hidden activations [Mp,Hcp]
  float* alb;     // [Mp,4]   albedo (network output)
  // backward-only
  float* u[RNB_MAX_LIN];   // RA sweep inputs u_l  (u[0] is [Mp,Ep])
  float* zR[RNB_MAX_LIN];  // second-order term entering layer l's pre-activation adjoint
  float* zb[RNB_MAX_LIN];  // pre-activation adjoints of F
  float* geb;     // [Mp,Ep]  adjoint of ge
  float* zc[RNB_MAX_LIN];  // albedo-net pre-activation adjoints
  float* cinb;    // [Mp,Cinp] adjoint of cin
  float* sbar;    // [Mp]
  float* nbar;    // [Mp,4]
  float* albbar;  // [Mp,4]
  void* u0_k8;              // RNB_VARIANT_BF16: u_0 = J_pe nbar as bf16 K8 [Mp,Ep]   (written by the RA sweep)
  void* cin8;               // RNB_VARIANT_BF16, bf16 albedo path: albedo-net input as bf16 K8 [Mp,Cinp]
  void* ac8[RNB_MAX_LIN];   //   hidden activations as bf16 K8 [Mp,256]
  void* zc8[RNB_MAX_LIN];   //   pre-activation adjoints as bf16 K8 [Mp,256]
  void* fbar_k8;            // RNB_VARIANT_BF16: feature part of cinb as bf16 K8 [Mp,256] (written by the FB sweep)
  unsigned* amax;           // [AMAX_SLOTS] max |.| of the adjoint tensors (float bits; zeroed at the start of a backward)
  unsigned* smax;           // [SMAX_SLOTS] max |.| of the saved forward state the x2h weight-gradient jobs take as operands
                            // (float bits; zeroed by the first kernel of a render forward, grown by the forward sweeps)
  float* dw_part;           // partial slabs of the split-K weight-gradient GEMMs: [deterministic variant | staged kernel]
  int64_t dw_part_floats;
  int64_t dw_slab_off;      // where the second part begins (floats): set with the buffer, read by dw_zero_partials / dw_backward
  unsigned* ac0_mask;       // fused albedo kernels: relu'(ac_0) as bits [tiles][256][2] (color_h2.hip)
  unsigned* alb_dead;       // fused albedo backward: one word per 64-point tile, 1 = the tile's colour adjoint is exactly zero and
  int64_t alb_dead_stride;  // the tile was skipped: no product ran, its zc_l and cinb rows are NOT written (BwdParts::dead_dw; else
                            // they hold stored zeros), and FB and the weight-gradient jobs skip the tile by this word.  Tile t's word is alb_dead[t * alb_dead_stride]: it lies in cinb, in the first
                            // encoding column of the tile's first row — columns F .. of cinb are written and read only by a
                            // backward that leaves the input adjoints (BwdParts::color_inputs), which never skips a tile
  float* col_part;          // fused albedo backward: per-tile column sums of the output layer's gradient [tiles][Co][256] + [tiles][Co]
  float* sdfh_part;         // sdf-head row gradient: per-slab column sums [kSdfHeadSlabs][Hp] + [kSdfHeadSlabs]
};

// slots of PointBufs::amax: zb_l, u_l (u_0 = geb), zc_l, cinb
// AMAX_DEAD_RAN (no maximum): set to 1 by the fused albedo backward when its zero-tile path was on, i.e. when the words of
// PointBufs::alb_dead were written by this backward (zeroed with the slots at the start of every backward); AMAX_ANY_DEAD: set to
// 1 by every tile that took the path — while it is 0 the weight-gradient kernel does not even look at the tiles' words
enum { AMAX_ZB = 0, AMAX_U = RNB_MAX_LIN, AMAX_ZC = 2 * RNB_MAX_LIN + 1, AMAX_CINB = 3 * RNB_MAX_LIN + 1, AMAX_MAXIMA = 3 * RNB_MAX_LIN + 2,
       AMAX_DEAD_RAN = AMAX_MAXIMA, AMAX_ANY_DEAD = AMAX_MAXIMA + 1, AMAX_SLOTS = AMAX_MAXIMA + 2 };
static_assert(AMAX_SLOTS * sizeof(unsigned) <= 256, "the slots fit the 256 bytes carve_points has always taken for them");
// slots of PointBufs::smax: a_l, gz_l (hidden layers), e (positional encoding), cin (albedo-net input), ac_l (its hidden layers);
// SMAX_NONFIN: raised to 1 by the fused albedo forward when a value of cin, ac_0 or ac_1 is an infinity or a NaN (the backward's
// zero-tile path then stays off for the step: 0 x that value is not zero)
enum { SMAX_A = 0, SMAX_GZ = RNB_MAX_LIN, SMAX_E = 2 * RNB_MAX_LIN, SMAX_CIN = 2 * RNB_MAX_LIN + 1, SMAX_AC = 2 * RNB_MAX_LIN + 2,
       SMAX_NONFIN = 3 * RNB_MAX_LIN + 2, SMAX_SLOTS = 3 * RNB_MAX_LIN + 3 };
static_assert(SMAX_SLOTS * sizeof(unsigned) <= 256, "the slots fit the 256 bytes carve_points has always taken for them");
// slot i of an x2h maxima array (PointBufs::amax / ::smax) when the route records them, else nullptr (also for the
// buffer-less PointBufs of a sizing query): a weight-gradient job then scales by the fixed 2^6, a GEMM records no maximum
inline unsigned* h2_slot(const Layout& L, unsigned* slots, int i) { return L.route.h2 && slots != nullptr ? slots + i : nullptr; }
// PM_NO_REVERSE: a backward without the normal's adjoint (point-wise autograd of SDFNetwork.forward): no gz_l, no u_l
enum PointMode { PM_SDF_ONLY = 0, PM_WITH_NORMAL = 1, PM_WITH_COLOR = 2, PM_WITH_BACKWARD = 4, PM_NO_REVERSE = 8 };
void carve_points(const Layout& L, Carver& c, int64_t M, int mode, PointBufs* pb);

// ---- the per-layer route (layers.hip): one GEMM launch per layer, any shape ---------------------
int launch_pe_points(const Layout& L, const float* pts, int64_t M, PointBufs& pb, hipStream_t s);
int sweep_forward(const Layout& L, const float* packed, PointBufs& pb, bool need_feat, bool need_gz_last,
                  float* feat_dense, hipStream_t s);
int sweep_reverse(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s);
int sweep_color(const Layout& L, const float* packed, PointBufs& pb, const float* pts, const float* nrm, int nrm_ld,
                hipStream_t s);
// its backward stages, in the shape of their fused counterparts (color_h2_backward, fused_ra, fused_fb)
int layers_color_backward(const Layout& L, const float* packed, PointBufs& pb, float* packed_grad, hipStream_t s);
int layers_ra(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s);
int layers_fb(const Layout& L, const float* packed, PointBufs& pb, bool with_feat, hipStream_t s);
// ebar = d loss / d e after an SDF backward of any fp32 route (into pb.geb, free after the backward); returns pb.geb
int launch_sdf_ebar(const Layout& L, const float* packed, PointBufs& pb, float** ebar, hipStream_t s);

// ---- small utility launches (util.hip) --------------------------------------------------------------
int launch_copy_cols(const float* src, int ld, int ncols, int64_t M, float* out, hipStream_t s);
int launch_fill_cols(const float* src, int ncols, int64_t M, int64_t Mp, int ld, float* dst, hipStream_t s);
int launch_grid_points(const GridGen& g, int64_t first, int64_t n, float* pts, hipStream_t s);
int launch_scale_copy(const float* src, float scale, int64_t n, float* dst, hipStream_t s);
int launch_grid_scatter(const GridGen& g, const float* src, int64_t first, int64_t n, float* dst, hipStream_t s);

// ---- per-vertex mesh attributes (mesh_attrs.hip): the kernels around the point sweeps of rnb_mesh_vertex_attrs --------
// where a chunk's points come from: grid-index float64 vertices (rescaled to the box: v / rm1 * span + bmin in float64,
// span = bound_max - bound_min in fp32) or fp32 points (copied)
struct MeshPointsSrc {
  const double* grid;   // [V,3] or nullptr
  const float* pts;     // [V,3], read when grid is nullptr
  double rm1;           // resolution - 1
  float span[3], bmin[3];
};
struct MeshOut {        // rnb_mesh_vertex_args' outputs (each may be nullptr)
  float* points;
  float* sdf;
  float* gradient;
  float* normal;
  float* albedo;
  uint8_t* rgb;
  int Co;               // albedo width (col_d_out)
  int swap_rb;
};
// vertices [first, first + n) -> pts [n,3]
int launch_mesh_points(const MeshPointsSrc& src, int64_t first, int64_t n, float* pts, hipStream_t s);
// one Newton step of pts [n,3] towards sdf = level, from the sweeps' sdf [n] and d sdf / d x [n,4]
int launch_mesh_newton(const float* sdf, const float* nrm, int64_t n, float level, float max_step, float* pts, hipStream_t s);
// rows [0, n) of the chunk's state (pb.sdf, pb.nrm, pb.alb) -> vertices [first, first + n) of the outputs
int launch_mesh_attrs(const float* pts, const PointBufs& pb, int64_t first, int64_t n, const MeshOut& o, hipStream_t s);

// ---- sparse SDF grid (sparse_grid.hip): brick bookkeeping around the forward sweeps' brick mode --------
struct SparseGeom {
  int res, bs, nb, nl;   // grid samples, cells per brick edge, bricks and lattice points (nb + 1) per axis
  float thr;             // "inside" = value <= thr, as marching cubes has it
  float seed_dist;       // a corner closer to thr than this makes its bricks seeds (margin x half a brick diagonal)
};
// state: one byte per brick (0 = not listed, 1 = listed) in whole 32-bit words; list: brick ids in listing order;
// n_listed: device counter (the list's length), read by the host between rounds
int launch_sparse_classify(const SparseGeom& sg, const float* lattice, uint32_t* state, int32_t* list, int64_t* n_listed,
                           hipStream_t s);
int launch_sparse_grow(const SparseGeom& sg, const float* volume, int64_t first, int64_t count, uint32_t* state, int32_t* list,
                       int64_t* n_listed, hipStream_t s);
int launch_sparse_fill(const SparseGeom& sg, const float* lattice, const uint32_t* state, float* volume, hipStream_t s);
int launch_absmax_rows(const float* x, int64_t n, unsigned* slot, hipStream_t s);
int launch_range_report(const Layout& L, const float* packed, const PointBufs& pb, bool with_color, bool with_backward, float* out,
                        hipStream_t s);

// ---- the backward of every route (backward.hip) -----------------------------------------------------
// which parts of the backward run
struct BwdParts {
  bool albedo;         // the albedo net's backward from pb.albbar
  bool sdf;            // the SDF network's backward from pb.sbar (+ the two below)
  bool feat;           // cinb's feature columns seed FB (the feature head's adjoint)
  bool normal;         // pb.nbar is live: geb, RA and the gz/u weight-gradient pairs
  bool color_inputs;   // leave all of cinb, encoding columns included, for the input adjoints
  bool dead_tiles = false;   // set by sweep_backward_parts (dead_tiles_on): the albedo backward skips tiles whose colour adjoint
                             // is exactly zero, and FB skips them with it
  bool dead_dw = false;      // ... and so do the weight-gradient jobs (dw_honours_dead): the tiles' zc_l / cinb rows then stay
                             // unwritten; else the albedo backward stores zeros in the rows those jobs read
  // a render's backward; the SDF network alone (SDFNetwork.forward / .gradient); the albedo net alone (RenderingNetwork)
  static BwdParts render(bool with_color, bool keep_color_inputs) { return {with_color, true, with_color, true, keep_color_inputs}; }
  static BwdParts sdf_points(bool feat, bool normal) { return {false, true, feat, normal, false}; }
  static BwdParts color_points(bool inputs) { return {true, false, false, false, inputs}; }
};
int sweep_backward(const Layout& L, const float* packed, PointBufs& pb, bool with_color, float* packed_grad, hipStream_t s);
int sweep_backward_parts(const Layout& L, const float* packed, PointBufs& pb, const BwdParts& parts, float* packed_grad,
                         hipStream_t s);
// input adjoints of the point-wise autograd calls
int launch_sdf_xbar(const Layout& L, const float* packed, PointBufs& pb, bool with_normal, float* xbar, hipStream_t s);
int launch_color_input_bwd(const Layout& L, const PointBufs& pb, float* pts_bar, float* nrm_bar, hipStream_t s);
// ---- weight-gradient jobs of a backward (dw.hip) ----
// floats of PointBufs::dw_part (carve_points) for a backward over M points, and the offset of its second part
int64_t dw_workspace_floats(const Layout& L, int64_t M, bool with_color, int64_t* slab_off);
// the one-workgroup-per-gradient kernel runs for this variant over M points (its slab reduction then sums the sdf-head row)
bool dw_one_wg_runs(const Layout& L, int64_t M);
// zeroes the deterministic variant's ordered-reduction slabs (before the backward's first launch)
int dw_zero_partials(const Layout& L, const PointBufs& pb, hipStream_t s);
// queues and launches every weight-gradient job of a backward of these parts (its other launches are enqueued)
int dw_backward(const Layout& L, const PointBufs& pb, const BwdParts& parts, int sdfh_slabs, float* packed_grad, hipStream_t s);
// every job that reads zc_l or cinb goes to the kernel that skips dead tiles (gemm_dw_x3_kernel)
bool dw_honours_dead(const Layout& L, int64_t M);
// FB runs as fused_fb_h2_kernel, which skips the feature-head seed of a dead tile
bool fused_fb_honours_dead(const Layout& L);
// the zero-tile path runs in a backward of these parts (RNB_VARIANT_NO_DEAD_TILES switches it off)
bool dead_tiles_on(const Layout& L, const PointBufs& pb, const BwdParts& parts);
int fused_reverse(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s, bool store_ge = false);
int fused_ra(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s, int* u_tiles = nullptr);
int fused_fb(const Layout& L, const float* packed, PointBufs& pb, bool with_color, hipStream_t s, bool dead_tiles = false);

// ---- fused sweeps for hidden width 256 (fused.hip) ---------------------------------------------------
bool fused_supported(const Layout& L);
int fused_forward(const Layout& L, const float* packed, const float* pts, int64_t M, PointBufs& pb, bool save,
                  bool need_feat, hipStream_t s, const GridGen* grid = nullptr);
// ---- M/V sweeps (sweep_mv.hip): x3 arithmetic, matrix waves (32 points each, transposed product, weights through an
// LDS-DMA ring) + vector waves (epilogues, saved state, operand split) ----
bool sweep_mv_supported(const Layout& L);
int sweep_mv_forward(const Layout& L, const float* packed, const float* pts, int64_t M, PointBufs& pb, bool save,
                     bool need_feat, hipStream_t s, const GridGen* grid = nullptr);
// family of a sweep over Mp points: the M/V kernels need >= one 128-point workgroup per CU to fill the chip
constexpr bool kRegTileDefault = false;
inline bool use_reg_tile(const Layout& L, int64_t Mp) {
  if (!sweep_mv_supported(L) || (L.variant & RNB_VARIANT_LDS_TILE)) return false;
  if (L.variant & RNB_VARIANT_REG_TILE) return true;
  return kRegTileDefault && Mp >= 128 * 200;
}

// ---- RNB_VARIANT_X3: fp32 products as six bf16 MFMA terms (fused_common.hip.h); the split weight mirror ----
inline bool is_x3(const Layout& L) { return (L.variant & RNB_VARIANT_X3) != 0; }
inline bool is_x2h(const Layout& L) { return is_x3(L) && (L.variant & RNB_VARIANT_X2H) != 0; }
// the fp16 two-plane mirror (RNB_VARIANT_X2H) behind the three bf16 planes: matrix at 2 x its float offset, in 2-byte units
inline unsigned short* x2h_mirror(const Layout& L, float* packed) {
  return reinterpret_cast<unsigned short*>(packed + L.total + L.total / 2 * 3);
}
inline const unsigned short* x2h_mirror(const Layout& L, const float* packed) {
  return reinterpret_cast<const unsigned short*>(packed + L.total + L.total / 2 * 3);
}
inline const H2Tab* h2_tab(const Layout& L, const float* packed) {
  return L.h2tab_off >= 0 ? reinterpret_cast<const H2Tab*>(packed + L.h2tab_off) : nullptr;
}
inline H2Tab* h2_tab(const Layout& L, float* packed) {
  return L.h2tab_off >= 0 ? reinterpret_cast<H2Tab*>(packed + L.h2tab_off) : nullptr;
}
int x3_pack_weights(const Layout& L, float* packed, hipStream_t s);

// ---- the albedo network as two fused sweeps in the x2h arithmetic (color_h2.hip) ----
bool color_h2_supported(const Layout& L);
int color_h2_forward(const Layout& L, const float* packed, PointBufs& pb, const float* pts, const float* nrm, hipStream_t s);
// sdf == false: no geb (the albedo net alone); keep_pe: also store cinb's 64 encoding columns (input adjoints)
int color_h2_backward(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s, bool sdf = true, bool keep_pe = false,
                      bool dead_tiles = false, bool dead_zero_fill = false);
int64_t color_h2_part_floats(const Layout& L, int64_t M);
constexpr int kSdfHeadSlabs = 64;   // row slabs of sdf_head_bwd_kernel's partial sums (summed in slab order: no atomics)

// ---- RNB_VARIANT_BF16 (bf16_common.hip.h): bf16-operand sweeps of the 256-wide network, saved state in bf16 "K8" layout ----
inline bool is_bf16(const Layout& L) { return (L.variant & RNB_VARIANT_BF16) != 0; }
// bf16_sweeps.hip: the weight mirror and the SDF network's sweeps
int bf16_pack_weights(const Layout& L, float* packed, hipStream_t s);
int bf16_forward(const Layout& L, const float* packed, const float* pts, int64_t M, PointBufs& pb, bool save, bool need_feat,
                 hipStream_t s, const GridGen* grid = nullptr, bool feat_k8 = false);
int bf16_reverse(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s);
int bf16_ra(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s);
int bf16_fb(const Layout& L, const float* packed, PointBufs& pb, bool with_color, hipStream_t s);
// bf16_color.hip: the albedo network
bool bf16_color_supported(const Layout& L);
int bf16_color_forward(const Layout& L, const float* packed, PointBufs& pb, const float* pts, hipStream_t s);
int bf16_color_backward(const Layout& L, const float* packed, PointBufs& pb, float* packed_grad, hipStream_t s);
// bf16_dw.hip: the sdf-head row's gradient and the grouped weight-gradient launch
int bf16_sdf_head_bwd(const Layout& L, PointBufs& pb, float* packed_grad, hipStream_t s);
int bf16_dw_backward(const Layout& L, PointBufs& pb, bool with_color, float* packed_grad, hipStream_t s);
// floats of bf16_dw_backward's ordered-reduction slabs over M points (deterministic variant)
int64_t bf16_dw_floats(const Layout& L, int64_t M, bool with_color);
// the two networks as the plan of that launch reads them (bf16_dw_plan.h)
inline BfDwNet bf16_dw_net(const Layout& L) {
  BfDwNet n{};
  n.nh = L.nh;
  for (int l = 0; l < L.nh; ++l) n.hid_Kp[l] = L.hid[l].Kp;
  n.feat_Kp = L.feat.Kp;
  n.bf16_color = L.route.color == COLOR_BF16;
  n.nc = L.nc;
  for (int l = 0; l < L.nc; ++l) n.col_Kp[l] = L.col[l].Kp;
  n.Cinp = L.Cinp;
  return n;
}

// ---- sampling / composite ------------------------------------------------------------------------
int launch_up_sample_step(const float* rays_o, const float* rays_d, const float* z_in, const float* sdf_old,
                          const float* sdf_new, const int32_t* gather_index, int n_old_for_gather,
                          int64_t B, int n, int n_new, float inv_s, float* new_z, int32_t* inds,
                          float* z_out, int32_t* sort_index, float* new_pts, float* sdf_sorted_out,
                          hipStream_t s);

// ---- composite (composite.hip) -------------------------------------------------------------------
struct CompArgs {
  int64_t B;
  int S, L, C;
  int flags;
  float cos_anneal;
  const float* rays_d;
  const float* pts;       // [B*S,3]
  const float* dists;     // [B,S]
  const float* sdf;       // [Mp]
  const float* nrm;       // [Mp,4]
  const float* alb;       // [Mp,4] (network output)
  const float* lights;    // [L,3] or [L,B,3]
  const float* bg;        // [3] or nullptr
  const float* variance;
  // forward outputs
  float* color_fine;
  float* weights;
  float* cdf;
  float* gradients;
  float* inside;
  float* weight_sum;
  float* weight_max;
  float* s_val;
  float* gerr_part;       // [B,2]
  float* gerr;            // [1] gradient_error, gerr_den [1] its denominator, gerr_partial [2] or nullptr: this shard's sums
  float* gerr_den;
  float* gerr_partial;
  float* sdf_out;         // optional copies
  float* albedo_out;
};

struct CompBwdArgs {
  CompArgs f;
  const float* weights;      // saved forward weights [B,S]
  const float* g_color;      // cotangents (nullable)
  const float* g_weights;
  const float* g_cdf;
  const float* g_gradients;
  const float* g_weight_sum;
  const float* g_weight_max;
  const float* g_s_val;
  const float* g_gerr;
  const float* gerr_den;     // [1]
  const float* gerr_den_global;   // [1] or nullptr: denominator of the whole data-parallel batch
  float* sbar;               // [Mp]
  float* nbar;               // [Mp,4]
  float* albbar;             // [Mp,4]
  float* invs_part;          // [B] partial d loss / d inv_s
  float* dvar;               // [1] d loss / d variance
  unsigned* amax_to_zero;    // PointBufs::amax (AMAX_SLOTS words) zeroed by the first workgroup, or nullptr
  // input adjoints (rnb_render_bwd_inputs), each nullptr = not wanted
  float* ig_cos_d;           // [B,3]   sum_s cosbar_s n_s: rays_d's part through true_cos
  float* ig_light;           // [L,B,3] sum_s shbar_s n_s per light and ray
  float* ig_bg;              // [B,3]   colour cotangent * (1 - sum w)
  float* ig_dists;           // [B,S]   d loss / d dists through the alpha estimate
};

// rnb_render_maps: the inputs of CompArgs; of its outputs only color_fine, weight_sum and weight_max are written (each may
// be nullptr), the per-sample ones are never touched
struct CompMapsArgs {
  CompArgs f;
  const float* z;          // [B,S] (depth)
  float* normal;           // [B,3] or nullptr
  float* albedo;           // [B,C] or nullptr
  float* depth;            // [B] or nullptr
};

int launch_fine_points(const float* rays_o, const float* rays_d, const float* z, int64_t B, int S, float sample_dist,
                       float* pts, float* dists, unsigned* smax_to_zero, hipStream_t s);
int launch_composite_fwd(const CompArgs& a, hipStream_t s);
int launch_composite_maps(const CompMapsArgs& g, hipStream_t s);
int launch_composite_bwd(const CompBwdArgs& g, hipStream_t s);
// limits of the per-ray kernels, defined once: composite.hip sizes its LDS rows and light registers by them, and api.hip
// refuses a larger S or light count in the workspace query and in render_setup, before anything is launched
constexpr int kMaxS = 512;               // samples per ray of the fine pass
constexpr int kMaxRenderLights = 8;
// per-ray reduction of the point adjoints pbar = d loss / d pts (rnb_render_bwd_inputs): pbar is formed per sample from
// the SDF network's encoding adjoint ebar, the Hessian term (d sdf / d e with the total normal adjoint) and the albedo
// net's encoded point / normal columns of cinb, and reduced into o_bar, d_bar (+ cos_d) and z_bar (with dists_bar)
struct RayAdjArgs {
  int64_t B;
  int S;
  const float* pts;        // [B*S,3] sample points (the albedo net's input)
  const float* dists;      // [B*S]
  const float* z;          // [B,S]
  const float* rays_d;     // [B,3]
  const float* x4;         // [Mp,4] scaled points
  const float* ebar;       // [Mp,Ep] d loss / d e
  const float* ge;         // [Mp,Ep] d sdf / d e
  const float* nbar;       // [Mp,4] the composite's normal adjoint
  const float* nrm;        // [Mp,4]
  const float* cinb;       // [Mp,Cinp] albedo-net input adjoint (encoding columns complete), or nullptr (no albedo net)
  int Ep, multires, Cinp, F, pev, multires_view;
  float scale;
  const float* cos_d;      // [B,3] or nullptr
  const float* dists_bar;  // [B,S] or nullptr (needed with z_bar)
  float* o_bar;            // [B,3] or nullptr
  float* d_bar;            // [B,3] or nullptr
  float* z_bar;            // [B,S] or nullptr
};
int launch_ray_input_adjoint(const RayAdjArgs& r, hipStream_t s);
// out[v*3 + c] = sum_b part[(v*B + b)*3 + c] for v < nvec, in a fixed order
int launch_sum_over_rays(const float* part, int64_t B, int nvec, float* out, hipStream_t s);

// ---- sampling (sampling.hip) ---------------------------------------------------------------------
// limits of up_sample_kernel (its LDS rows; one lane per new depth), also checked up front by api.hip check_sampling_desc
constexpr int kMaxZ = 512;    // n + n_new upper bound
constexpr int kMaxNew = 64;
int launch_z_init(const float* rays_o, const float* rays_d, const float* near, const float* far,
                  const float* t_rand, int64_t B, int n, float* z, float* pts, hipStream_t s);
int launch_gather_sdf(const float* sdf_old, const float* sdf_new, const int32_t* index, int64_t B, int n, int n_new,
                      float* out, hipStream_t s);

// ---- weight norm (weightnorm.hip) ------------------------------------------------------------------
int weightnorm_fwd(const rnb_model_desc* d, const Layout& L, const rnb_mlp_params* sdf, const rnb_mlp_params* color,
                   float* packed, hipStream_t s);
int weightnorm_bwd(const rnb_model_desc* d, const Layout& L, const rnb_mlp_params* sdf, const rnb_mlp_params* color,
                   const float* pgrad, const rnb_mlp_grads* gs, const rnb_mlp_grads* gc, hipStream_t s);
const char* last_error();

// ---- optional GEMM event instrumentation (prof.hip) ----------------------------------------------
bool prof_enabled();
void prof_begin(double flops, hipStream_t s, const char* tag);
void prof_end(hipStream_t s);
int profile_enable(int on);
int profile_collect(double* ms, int64_t* launches, double* flops);
int64_t profile_report(char* out, int64_t cap);
struct ProfScope {
  hipStream_t s;
  bool on;
  // tag: kernel class for the per-class report (a string literal: it is kept by pointer)
  ProfScope(double flops, hipStream_t st, const char* tag = nullptr) : s(st), on(prof_enabled()) {
    if (on) prof_begin(flops, s, tag);
  }
  ~ProfScope() {
    if (on) prof_end(s);
  }
};

}  // namespace rnb
