// The per-layer route of both networks (SDF_LAYERS / COLOR_LAYERS): one GEMM launch per layer with the layer's point-wise
// work in its epilogue, for any shape.  Forward (F), reverse-mode normal (R), albedo MLP (C) and the stages of the explicit
// backward (C', RA, FB) that backward.hip strings together -- see oracle/explicit.py for the mathematical statement and the
// reference lines each stage replaces (models/fields.py:82-127, :177-215; the backward replaces autograd's double backward
// invoked at exp_runner.py:261).  The input adjoint's two products (launch_sdf_ebar) run here on every fp32 route.
#include "gemm.hip.h"
#include "pe.hip.h"
#include "rnb_internal.h"

namespace rnb {

// =====================================================================================================
// point-wise kernels
// =====================================================================================================

// positional encoding (models/embedder.py:40-46): e = [x, sin(2^k x), cos(2^k x)]_k, padded with zeros
__global__ void pe_points_kernel(const float* __restrict__ pts, int64_t M, int64_t Mp, float scale, int multires,
                                 int Ep, float* __restrict__ x4, float* __restrict__ e) {
  int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= Mp) return;
  float x[3] = {0.f, 0.f, 0.f};
  if (row < M) {
    x[0] = pts[row * 3 + 0] * scale;
    x[1] = pts[row * 3 + 1] * scale;
    x[2] = pts[row * 3 + 2] * scale;
  }
  x4[row * 4 + 0] = x[0]; x4[row * 4 + 1] = x[1]; x4[row * 4 + 2] = x[2]; x4[row * 4 + 3] = 0.f;
  float* er = e + row * Ep;
  er[0] = x[0]; er[1] = x[1]; er[2] = x[2];
  pe_sincos(x, multires, 0, 1, [&](int c, float s, float co) {
    er[c] = s;
    er[c + 3] = co;
  });
  for (int c = 3 + 6 * multires; c < Ep; ++c) er[c] = 0.f;
}

// sdf head: sdf = (a_last . w_sdf + b_sdf)/scale ; optionally seeds the reverse sweep gz_last = w_sdf * D
// 32 lanes per point.
__global__ void sdf_head_kernel(const float* __restrict__ a, const float* __restrict__ D, int Hp, int H,
                                const float* __restrict__ wsdf, const float* __restrict__ bsdf, float inv_scale,
                                int64_t Mp, float* __restrict__ sdf, float* __restrict__ gz) {
  const int sub = threadIdx.x & 31;
  int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
  if (row >= Mp) return;
  const float* ar = a + row * Hp;
  float acc = 0.f;
  for (int k = sub; k < Hp; k += 32) {
    const float av = ar[k];
    const float w = k < H ? wsdf[k] : 0.f;
    acc = fmaf(av, w, acc);
    if (gz) gz[row * Hp + k] = k < H ? w * D[row * Hp + k] : 0.f;
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 32);
  if (sub == 0) sdf[row] = (acc + bsdf[0]) * inv_scale;
}

// normal = J_pe(x)^T g_e   (d sdf / d pts; models/fields.py:114-127)
__global__ void normal_kernel(const float* __restrict__ x4, const float* __restrict__ ge, int Ep, int multires,
                              int64_t Mp, float* __restrict__ nrm) {
  int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= Mp) return;
  const float* g = ge + row * Ep;
  float n[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) n[d] = g[d];
  pe_adjoint(x4 + row * 4, g, multires, 0, 1, n);
  nrm[row * 4 + 0] = n[0]; nrm[row * 4 + 1] = n[1]; nrm[row * 4 + 2] = n[2]; nrm[row * 4 + 3] = 0.f;
}

// albedo-net input columns F.. : [pe_v(p) | pe_v(n) | 0]  (feature columns 0..F-1 are written by the
// feature-head GEMM).  models/fields.py:179-191 in the packed column order.  One wave = 64 points;
// dynamic LDS = 64 * (Cinp - F + 1) floats.
__global__ __launch_bounds__(64) void color_input_kernel(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                         int nrm_ld, int64_t M, int64_t Mp, int F, int multires,
                                                         int Cinp, float* __restrict__ cin) {
  extern __shared__ float tile[];
  const int lane = threadIdx.x, W = Cinp - F;
  const int64_t r0 = (int64_t)blockIdx.x * 64, row = r0 + lane;
  const int pev = 3 + 6 * multires;
  for (int which = 0; which < 2; ++which) {
    float* cr = tile + lane * (W + 1) + which * pev;
    float v[3] = {0.f, 0.f, 0.f};
    if (row < M) {
      if (which == 0) { v[0] = pts[row * 3]; v[1] = pts[row * 3 + 1]; v[2] = pts[row * 3 + 2]; }
      else { v[0] = nrm[row * nrm_ld]; v[1] = nrm[row * nrm_ld + 1]; v[2] = nrm[row * nrm_ld + 2]; }
    }
    cr[0] = v[0]; cr[1] = v[1]; cr[2] = v[2];
    pe_sincos(v, multires, 0, 1, [&](int c, float s, float co) {
      cr[c] = s;
      cr[c + 3] = co;
    });
  }
  for (int c = 2 * pev; c < W; ++c) tile[lane * (W + 1) + c] = 0.f;
  __builtin_amdgcn_wave_barrier();
  tile_store64(cin, Cinp, r0, F, W, tile, lane);
}

// albedo output layer (d_out rows) + sigmoid: 32 lanes per point.
// One wave per 4 rows: lane l reads the float4 l (+ 64, ..) of a row — a whole 1 KB row per load instruction, four rows
// in flight — and keeps the output layer's <= 4 weight rows for its columns in registers (Hcp <= 256 * 4).
__global__ __launch_bounds__(256) void color_out_kernel(const float* __restrict__ ac, int Hcp, int Hc, const float* __restrict__ Wo,
                                 int ldwo, const float* __restrict__ bo, int Co, int squeeze, int64_t Mp,
                                 float* __restrict__ alb) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t row0 = wave * 4;
  if (row0 >= Mp) return;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  for (int k4 = lane; k4 * 4 < Hcp; k4 += 64) {
    vf4 w[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      w[c] = make_vf4(0.f, 0.f, 0.f, 0.f);
      if (c < Co) {
        const float* wp = Wo + (size_t)c * ldwo + k4 * 4;
        w[c] = make_vf4(k4 * 4 < Hc ? wp[0] : 0.f, k4 * 4 + 1 < Hc ? wp[1] : 0.f, k4 * 4 + 2 < Hc ? wp[2] : 0.f,
                        k4 * 4 + 3 < Hc ? wp[3] : 0.f);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (row0 + r < Mp) {
        const vf4 a = *reinterpret_cast<const vf4*>(ac + (row0 + r) * Hcp + k4 * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[r][c] = fmaf(a.x, w[c].x, fmaf(a.y, w[c].y, fmaf(a.z, w[c].z, fmaf(a.w, w[c].w, acc[r][c]))));
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[r][c] += __shfl_xor(acc[r][c], o, 64);
    }
  if (lane < 4 && row0 + lane < Mp) {   // lane r finishes row r
    const int64_t row = row0 + lane;
    float mine[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) mine[c] = lane == 0 ? acc[0][c] : lane == 1 ? acc[1][c] : lane == 2 ? acc[2][c] : acc[3][c];
    for (int c = 0; c < 4; ++c) {
      float v = 0.f;
      if (c < Co) {
        v = mine[c] + bo[c];
        if (squeeze) v = 1.f / (1.f + expf(-v));
      }
      alb[row * 4 + c] = v;
    }
  }
}

// backward of the albedo output layer: zo = albbar * alb(1-alb); zc_last = (zo Wo) * relu'(ac);
// dWo += zo^T ac ; dbo += sum zo.   A workgroup owns 32 columns (blockIdx.y) and a slab of rows (blockIdx.x):
// thread = (4 columns, one of 64 row phases); 16-byte accesses, one 128-byte line per row and matrix; an output
// address receives one atomic per row slab (same-address atomics serialise in the L2).  Co <= 4.
__global__ __launch_bounds__(512) void color_out_bwd_kernel(const float* __restrict__ albbar,
                                                            const float* __restrict__ alb,
                                                            const float* __restrict__ ac, int Hcp, int Hc,
                                                            const float* __restrict__ Wo, int ldwo, int Co,
                                                            int squeeze, int64_t M, int rows_per_blk,
                                                            float* __restrict__ zc, float* __restrict__ dWo,
                                                            float* __restrict__ dbo, unsigned* __restrict__ amax) {
  __shared__ float red[64][4][33];
  __shared__ float redb[64][4];
  const int tid = threadIdx.x, cg = tid & 7, ph = tid >> 3;
  const int kl = cg * 4, k0 = blockIdx.y * 32 + kl;
  const bool bias_blk = blockIdx.y == 0;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk;
  const int64_t r1 = min(M, r0 + rows_per_blk);
  float w[4][4], dw[4][4], db[4] = {0.f, 0.f, 0.f, 0.f};
  float zmax = 0.f;   // max |zc| written by this thread (rows < M only: the loop stops at r1)
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[c][j] = (c < Co && k0 + j < Hc) ? Wo[c * ldwo + k0 + j] : 0.f;
      dw[c][j] = 0.f;
    }
#pragma unroll 4
  for (int64_t row = r0 + ph; row < r1; row += 64) {
    const vf4 a4 = *reinterpret_cast<const vf4*>(alb + row * 4);
    const vf4 g4 = *reinterpret_cast<const vf4*>(albbar + row * 4);
    float zo[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) zo[c] = c < Co ? g4[c] * (squeeze ? a4[c] * (1.f - a4[c]) : 1.f) : 0.f;
    if (cg == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) db[c] += zo[c];
    }
    const vf4 av = *reinterpret_cast<const vf4*>(ac + row * Hcp + k0);
    vf4 z;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) { t = fmaf(zo[c], w[c][j], t); dw[c][j] = fmaf(zo[c], av[j], dw[c][j]); }
      z[j] = (k0 + j < Hc && av[j] > 0.f) ? t : 0.f;
      zmax = fmaxf(zmax, fabsf(z[j]));
    }
    *reinterpret_cast<vf4*>(zc + row * Hcp + k0) = z;
  }
  __shared__ float zm[8];
  if (amax != nullptr) {   // (uniform)  wave maxima meet in LDS behind the barrier below: one atomic per workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) zmax = fmaxf(zmax, __shfl_xor(zmax, o, 64));
    if ((tid & 63) == 0) zm[tid >> 6] = zmax;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[ph][c][kl + j] = dw[c][j];
  if (cg == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) redb[ph][c] = db[c];
  }
  __syncthreads();
  if (amax != nullptr && tid == 511) {
    float m = zm[0];
    for (int w = 1; w < 8; ++w) m = fmaxf(m, zm[w]);
    const unsigned b = __builtin_bit_cast(unsigned, m);
    if (b > __atomic_load_n(amax, __ATOMIC_RELAXED)) atomicMax(amax, b);
  }
  if (tid < 128) {            // (c, column) pairs of this chunk
    const int c = tid >> 5, col = tid & 31;
    float t = 0.f;
    for (int q = 0; q < 64; ++q) t += red[q][c][col];
    if (c < Co && blockIdx.y * 32 + col < Hc) atomicAdd(dWo + c * ldwo + blockIdx.y * 32 + col, t);
  } else if (bias_blk && tid < 128 + Co) {
    const int c = tid - 128;
    float t = 0.f;
    for (int q = 0; q < 64; ++q) t += redb[q][c];
    atomicAdd(dbo + c, t);
  }
}

// =====================================================================================================
// GEMM epilogues.  apply4(row, col, v): 4 consecutive columns col..col+3 (col % 4 == 0) of one output row.
// All activation matrices have a padded leading dimension (multiple of 32), so 16-byte accesses are
// aligned and in bounds; columns >= the real width are written as zeros (or the skip-connection payload).
// =====================================================================================================
__device__ inline vf4 ld4(const float* p) { return *reinterpret_cast<const vf4*>(p); }
__device__ inline void st4(float* p, vf4 v) { *reinterpret_cast<vf4*>(p) = v; }

// F hidden layer: a = softplus(acc + b), D = softplus'(acc + b); columns >= N_real: PE override (layer
// feeding the skip layer) or 0
struct EpiF {
  const float* b;
  float* out;
  float* outD;     // nullptr when no derivative is needed (no-grad SDF evaluation)
  int ld;
  int n_real;
  const float* e;  // nullptr unless this layer feeds the skip layer
  int Ep, pe;
  __device__ void apply4(int row, int col, vf4 v) const {
    const vf4 bb = ld4(b + col);
    vf4 a, D;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int cc = col + c;
      float ac, Dc;
      if (cc < n_real) softplus_aD(v[c] + bb[c], ac, Dc);
      else {
        ac = (e != nullptr && cc < n_real + pe) ? e[(size_t)row * Ep + (cc - n_real)] : 0.f;
        Dc = 0.f;
      }
      a[c] = ac;
      D[c] = Dc;
    }
    st4(out + (size_t)row * ld + col, a);
    if (outD) st4(outD + (size_t)row * ld + col, D);
  }
};
// plain linear head (+bias) written to a strided buffer for columns < n_real (n_real % 4 == 0 not assumed)
struct EpiBias {
  const float* b;
  float* out;
  int ld;
  int n_real;
  __device__ void apply4(int row, int col, vf4 v) const {
    if (col + 3 < n_real) {
      st4(out + (size_t)row * ld + col, v + ld4(b + col));
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (col + c < n_real) out[(size_t)row * ld + col + c] = v[c] + b[col + c];
    }
  }
};
struct EpiRelu {
  const float* b;
  float* out;
  int ld;
  int n_real;
  __device__ void apply4(int row, int col, vf4 v) const {
    const vf4 bb = ld4(b + col);
    vf4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = col + c < n_real ? relu_nan(v[c] + bb[c]) : 0.f;
    st4(out + (size_t)row * ld + col, o);
  }
};
// R layer l>=1: g = acc ; skip layer: columns [k_split, k_split+pe) go to ge ; gz_{l-1} = g * D_{l-1}
struct EpiR {
  const float* D_prev;
  float* gz_prev;
  int ld;
  int k_split;   // number of columns that belong to the previous layer's output
  float* ge;     // destination of the skip part (or nullptr)
  int Ep, pe;
  __device__ void apply4(int row, int col, vf4 v) const {
    const size_t o = (size_t)row * ld + col;
    if (col + 3 < k_split) {
      st4(gz_prev + o, v * ld4(D_prev + o));
    } else {
      vf4 g;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int cc = col + c;
        if (cc < k_split) g[c] = v[c] * D_prev[o + c];
        else {
          if (ge != nullptr && cc < k_split + pe) ge[(size_t)row * Ep + (cc - k_split)] = v[c];
          g[c] = 0.f;
        }
      }
      st4(gz_prev + o, g);
    }
  }
};
// R layer 0: ge (+)= acc
struct EpiR0 {
  float* ge;
  int Ep, pe;
  int accumulate;
  __device__ void apply4(int row, int col, vf4 v) const {
    const size_t o = (size_t)row * Ep + col;
    vf4 g = accumulate ? ld4(ge + o) : make_vf4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 4; ++c) g[c] = col + c < pe ? g[c] + v[c] : 0.f;
    st4(ge + o, g);
  }
};
// RA layer l: gzb = acc ; zR_l = 100 gzb gz_l (1 - D_l) ; u_{l+1} = gzb D_l  (PE-adjoint override when
// feeding the skip layer)
struct EpiRA {
  const float* D;
  const float* gz;
  float* zR;
  float* u_next;
  int ld;
  int n_real;
  const float* geb;  // nullptr unless this layer feeds the skip layer
  int Ep, pe;
  __device__ void apply4(int row, int col, vf4 v) const {
    const size_t o = (size_t)row * ld + col;
    const vf4 Dv = ld4(D + o), gzv = ld4(gz + o);
    vf4 zr, un;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int cc = col + c;
      if (cc < n_real) {
        zr[c] = 100.f * v[c] * gzv[c] * (1.f - Dv[c]);
        un[c] = v[c] * Dv[c];
      } else {
        zr[c] = 0.f;
        un[c] = (geb != nullptr && cc < n_real + pe) ? geb[(size_t)row * Ep + (cc - n_real)] : 0.f;
      }
    }
    st4(zR + o, zr);
    st4(u_next + o, un);
  }
};
// FB: zb_{l-1} = (acc [+ sbar/scale * w_sdf]) * D_{l-1} + zR_{l-1}
struct EpiFB {
  const float* D_prev;
  const float* zR_prev;
  float* zb_prev;
  int ld;
  int n_real;          // real width of layer l-1's output
  const float* sbar;   // only for the head step
  const float* wsdf;
  float inv_scale;
  __device__ void apply4(int row, int col, vf4 v) const {
    const size_t o = (size_t)row * ld + col;
    const vf4 Dv = ld4(D_prev + o), zr = ld4(zR_prev + o);
    if (sbar != nullptr) {
      const float sb = sbar[row] * inv_scale;
      const vf4 w = ld4(wsdf + col);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = fmaf(sb, w[c], v[c]);
    }
    vf4 zb;
#pragma unroll
    for (int c = 0; c < 4; ++c) zb[c] = col + c < n_real ? fmaf(v[c], Dv[c], zr[c]) : 0.f;
    st4(zb_prev + o, zb);
  }
};
// albedo backward through a relu layer: zc_{l-1} = acc * (ac_{l-1} > 0)
struct EpiReluMask {
  const float* ac_prev;
  float* out;
  int ld;
  int n_real;
  __device__ void apply4(int row, int col, vf4 v) const {
    const size_t o = (size_t)row * ld + col;
    const vf4 a = ld4(ac_prev + o);
    vf4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = (col + c < n_real && a[c] > 0.f) ? v[c] : 0.f;
    st4(out + o, r);
  }
};
struct EpiStore {
  float* out;
  int ld;
  __device__ void apply4(int row, int col, vf4 v) const { st4(out + (size_t)row * ld + col, v); }
};

// skip layer's encoding columns of zb_skip W_skip -> ebar (the first product of x's adjoint; layer 0's EpiR0 accumulates)
struct EpiSkipPE {
  float* ebar;
  int Ep, k_split, pe;
  __device__ void apply4(int row, int col, vf4 v) const {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int cc = col + c;
      if (cc >= k_split && cc < k_split + pe) ebar[(size_t)row * Ep + (cc - k_split)] = v[c];
    }
  }
};

// =====================================================================================================
// launch helpers
// =====================================================================================================

// x3: the product as six bf16 MFMA terms (RNB_VARIANT_X3; k-contiguous weights, N >= 256, K % 16 == 0)
template <bool B_KMAJOR, class Epi>
static int launch_rows(const float* A, int lda, const float* W, int ldw, int64_t Mp, int N, int K, const Epi& epi,
                       double flops, hipStream_t s, bool x3 = false, const x3raw* W3 = nullptr, unsigned* amax = nullptr,
                       int64_t m_real = 0, const char* tag = "layer_gemm") {
  ProfScope prof(flops, s, tag);
  if constexpr (!B_KMAJOR) {
    // W3: this matrix in the split mirror (x3_pack_weights): the weights are then read as ready-made fragments
    if (x3 && W3 != nullptr && N % 32 == 0 && N <= 512 && K % 32 == 0 && Mp % 128 == 0) {
      if (N <= 256) hipLaunchKernelGGL((gemm_rows_x3m_kernel<1, Epi>), dim3((unsigned)(Mp / 128)), dim3(512), 0, s, A, lda, W3, N, K, epi, amax, (long long)m_real);
      else hipLaunchKernelGGL((gemm_rows_x3m_kernel<2, Epi>), dim3((unsigned)(Mp / 128)), dim3(512), 0, s, A, lda, W3, N, K, epi, amax, (long long)m_real);
      RNB_CHECK_LAUNCH();
      return RNB_OK;
    }
    // (only the mirror kernels above leave max |.| of their outputs: a weight-gradient job scaled by a slot nobody wrote
    // would overflow — refuse instead of falling through)
    if (amax != nullptr) RNB_FAIL(RNB_E_INVALID, "layer GEMM %d x %d: the x2h maxima were requested from a kernel that does not record them", N, K);
    if (x3 && N >= 256 && K % XK == 0) {
      dim3 grid((unsigned)(Mp / BM), (unsigned)((N + 255) / 256));
      if (N % 256 == 0) hipLaunchKernelGGL((gemm_rows_x3_kernel<256, false, Epi>), grid, dim3(256), 0, s, A, lda, W, ldw, N, K, epi);
      else hipLaunchKernelGGL((gemm_rows_x3_kernel<256, true, Epi>), grid, dim3(256), 0, s, A, lda, W, ldw, N, K, epi);
      RNB_CHECK_LAUNCH();
      return RNB_OK;
    }
  }
  if (N >= 256) {   // 128 x 256 tiles: the 256-wide layers of the full model run as one wave of 2 blocks / CU
    dim3 grid((unsigned)(Mp / BM), (unsigned)((N + 255) / 256));
    if (N % 256 == 0)
      hipLaunchKernelGGL((gemm_rows_kernel<B_KMAJOR, 256, false, Epi>), grid, dim3(256), 0, s, A, lda, W, ldw, N, K, epi);
    else
      hipLaunchKernelGGL((gemm_rows_kernel<B_KMAJOR, 256, true, Epi>), grid, dim3(256), 0, s, A, lda, W, ldw, N, K, epi);
  } else {
    dim3 grid((unsigned)(Mp / BM), (unsigned)((N + 127) / 128));
    if (N % 128 == 0)
      hipLaunchKernelGGL((gemm_rows_kernel<B_KMAJOR, 128, false, Epi>), grid, dim3(256), 0, s, A, lda, W, ldw, N, K, epi);
    else
      hipLaunchKernelGGL((gemm_rows_kernel<B_KMAJOR, 128, true, Epi>), grid, dim3(256), 0, s, A, lda, W, ldw, N, K, epi);
  }
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// the split mirror of the matrix at float offset `off` of the packed buffer (x3_pack_weights), or nullptr
static inline const x3raw* x3_mirror(const Layout& L, const float* packed, int64_t off) {
  if (!is_x3(L) || off < 0) return nullptr;
  return reinterpret_cast<const x3raw*>(packed + L.total) + 3 * off;
}

int launch_pe_points(const Layout& L, const float* pts, int64_t M, PointBufs& pb, hipStream_t s) {
  hipLaunchKernelGGL(pe_points_kernel, dim3(blocks_for(pb.Mp, 256)), dim3(256), 0, s, pts, M, pb.Mp, L.sdf_scale,
                     L.multires, L.Ep, pb.x, pb.e);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// F: forward sweep (models/fields.py:82-104).  Needs pb.e; fills pb.a[*], pb.sdf, optionally the feature
// block of pb.cin (need_feat) and the reverse-sweep seed pb.gz[nh-1] (need_gz_last).
int sweep_forward(const Layout& L, const float* packed, PointBufs& pb, bool need_feat, bool need_gz_last,
                  float* feat_dense, hipStream_t s) {
  for (int l = 0; l < L.nh; ++l) {
    const Lin& ln = L.hid[l];
    const float* in = l == 0 ? pb.e : pb.a[l - 1];
    const int lda = l == 0 ? L.Ep : L.Hp;
    EpiF epi{packed + ln.b_off, pb.a[l], pb.D[l], L.Hp, ln.N, (l + 1 == L.skip) ? pb.e : nullptr, L.Ep, L.pe};
    RNB_TRY((launch_rows<false, EpiF>(in, lda, packed + ln.w_off, ln.Kp, pb.Mp, ln.Np, ln.Kp, epi, mm_flops(pb.M, ln), s)));
  }
  hipLaunchKernelGGL(sdf_head_kernel, dim3(blocks_for(pb.Mp * 32, 256)), dim3(256), 0, s, pb.a[L.nh - 1],
                     pb.D[L.nh - 1], L.Hp, L.H, packed + L.wsdf_off, packed + L.bsdf_off, 1.f / L.sdf_scale, pb.Mp, pb.sdf,
                     need_gz_last ? pb.gz[L.nh - 1] : nullptr);
  RNB_CHECK_LAUNCH();
  if (need_feat) {
    EpiBias epi{packed + L.feat.b_off, pb.cin, L.Cinp, L.F};
    RNB_TRY((launch_rows<false, EpiBias>(pb.a[L.nh - 1], L.Hp, packed + L.feat.w_off, L.feat.Kp, pb.Mp, L.feat.Np,
                                         L.feat.Kp, epi, mm_flops(pb.M, L.feat), s)));
    if (feat_dense) {
      RNB_TRY(launch_copy_cols(pb.cin, L.Cinp, L.F, pb.M, feat_dense, s));
    }
  }
  return RNB_OK;
}

// R: reverse sweep for the normal (models/fields.py:114-127 without autograd).  Needs pb.a[*], pb.gz[nh-1].
int sweep_reverse(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s) {
  for (int l = L.nh - 1; l >= 1; --l) {
    const Lin& ln = L.hid[l];
    const bool is_skip = (l == L.skip);
    EpiR epi{pb.D[l - 1], pb.gz[l - 1], L.Hp, is_skip ? ln.K - L.pe : ln.K, is_skip ? pb.ge : nullptr, L.Ep, L.pe};
    RNB_TRY((launch_rows<true, EpiR>(pb.gz[l], L.Hp, packed + ln.w_off, ln.Kp, pb.Mp, ln.Kp, ln.Np, epi, mm_flops(pb.M, ln), s)));
  }
  {
    const Lin& ln = L.hid[0];
    EpiR0 epi{pb.ge, L.Ep, L.pe, L.skip >= 1 ? 1 : 0};
    RNB_TRY((launch_rows<true, EpiR0>(pb.gz[0], L.Hp, packed + ln.w_off, ln.Kp, pb.Mp, ln.Kp, ln.Np, epi, mm_flops(pb.M, ln), s)));
  }
  hipLaunchKernelGGL(normal_kernel, dim3(blocks_for(pb.Mp, 256)), dim3(256), 0, s, pb.x, pb.ge, L.Ep, L.multires,
                     pb.Mp, pb.nrm);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// C: albedo network (models/fields.py:177-215, mode no_view_dir).  Needs the feature block of pb.cin and pb.nrm.
int sweep_color(const Layout& L, const float* packed, PointBufs& pb, const float* pts, const float* nrm, int nrm_ld,
                hipStream_t s) {
  hipLaunchKernelGGL(color_input_kernel, dim3(blocks_for(pb.Mp, 64)), dim3(64),
                     (size_t)64 * (L.Cinp - L.F + 1) * sizeof(float), s, pts, nrm, nrm_ld, pb.M, pb.Mp,
                     L.F, L.multires_view, L.Cinp, pb.cin);
  RNB_CHECK_LAUNCH();
  for (int l = 0; l < L.nc; ++l) {
    const Lin& ln = L.col[l];
    const float* in = l == 0 ? pb.cin : pb.ac[l - 1];
    const int lda = l == 0 ? L.Cinp : L.Hcp;
    EpiRelu epi{packed + ln.b_off, pb.ac[l], L.Hcp, ln.N};
    // (per-layer path of an albedo net the fused kernels do not cover: six bf16 terms — no operand range to look after)
    RNB_TRY((launch_rows<false, EpiRelu>(in, lda, packed + ln.w_off, ln.Kp, pb.Mp, ln.Np, ln.Kp, epi, mm_flops(pb.M, ln), s, is_x3(L),
                                         x3_mirror(L, packed, ln.w_off), nullptr, 0, "layer_gemm(forward)")));
    // x2h weight gradients take this layer's input / output as a state operand: its maximum (PointBufs::smax; a
    // forward-only call has none to keep)
    if (L.route.h2 && pb.smax != nullptr) {
      if (l == 0) RNB_TRY(launch_absmax_rows(pb.cin, pb.Mp * L.Cinp, pb.smax + SMAX_CIN, s));
      RNB_TRY(launch_absmax_rows(pb.ac[l], pb.Mp * L.Hcp, pb.smax + SMAX_AC + l, s));
    }
  }
  hipLaunchKernelGGL(color_out_kernel, dim3(blocks_for(pb.Mp * 16, 256)), dim3(256), 0, s, pb.ac[L.nc - 1], L.Hcp,
                     L.Hc, packed + L.colo.w_off, L.colo.Kp, packed + L.colo.b_off, L.Co, L.squeeze, pb.Mp, pb.alb);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// C': albedo network backward from pb.albbar.  Leaves zc_l and cinb; the output layer's gradient goes straight into
// packed_grad, the hidden layers' are weight-gradient jobs (dw.hip).
int layers_color_backward(const Layout& L, const float* packed, PointBufs& pb, float* packed_grad, hipStream_t s) {
  const int64_t M = pb.M, Mp = pb.Mp;
  const bool det = (L.variant & RNB_VARIANT_DETERMINISTIC) != 0;
  const int chunks = L.Hcp / 32;   // 32-column chunks x row slabs, ~256 workgroups, slabs a multiple of 64 rows
  int64_t slabs = det ? 1 : (256 + chunks - 1) / chunks;   // deterministic: ONE slab, i.e. one add per address onto zero
  int rows_per_blk = (int)((M + slabs - 1) / slabs);
  rows_per_blk = (rows_per_blk + 63) / 64 * 64;
  hipLaunchKernelGGL(color_out_bwd_kernel, dim3(blocks_for(M, rows_per_blk), chunks), dim3(512), 0, s, pb.albbar, pb.alb,
                     pb.ac[L.nc - 1], L.Hcp, L.Hc, packed + L.colo.w_off, L.colo.Kp, L.Co, L.squeeze, M,
                     rows_per_blk, pb.zc[L.nc - 1], packed_grad + L.colo.w_off, packed_grad + L.colo.b_off,
                     h2_slot(L, pb.amax, AMAX_ZC + L.nc - 1));
  RNB_CHECK_LAUNCH();
  for (int l = L.nc - 1; l >= 0; --l) {
    const Lin& ln = L.col[l];
    if (l > 0) {
      EpiReluMask epi{pb.ac[l - 1], pb.zc[l - 1], L.Hcp, L.col[l - 1].N};
      // zc_{l-1} = (zc_l W_l) * relu': k-contiguous product against the transposed copy W_l^T [Kp x Np]
      // (per-layer path: six bf16 terms; the kernel leaves max |acc| for the x2h weight-gradient job of zc_{l-1})
      RNB_TRY((launch_rows<false, EpiReluMask>(pb.zc[l], L.Hcp, packed + ln.wT_off, ln.Np, Mp, ln.Kp, ln.Np, epi, mm_flops(M, ln), s, is_x3(L),
                                               x3_mirror(L, packed, ln.wT_off), h2_slot(L, pb.amax, AMAX_ZC + l - 1), M)));
    } else {
      EpiStore epi{pb.cinb, L.Cinp};
      RNB_TRY((launch_rows<false, EpiStore>(pb.zc[0], L.Hcp, packed + ln.wT_off, ln.Np, Mp, ln.Kp, ln.Np, epi, mm_flops(M, ln), s, is_x3(L),
                                            x3_mirror(L, packed, ln.wT_off), h2_slot(L, pb.amax, AMAX_CINB), M)));
    }
  }
  return RNB_OK;
}

// RA: adjoint of the reverse sweep, forward layer order.  Needs pb.geb = u_0; leaves zR_l and u_{l+1}.
int layers_ra(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s) {
  for (int l = 0; l < L.nh; ++l) {
    const Lin& ln = L.hid[l];
    const float* in = l == 0 ? pb.geb : pb.u[l];
    const int lda = l == 0 ? L.Ep : L.Hp;
    EpiRA epi{pb.D[l], pb.gz[l], pb.zR[l], pb.u[l + 1], L.Hp, ln.N, (l + 1 == L.skip) ? pb.geb : nullptr, L.Ep, L.pe};
    RNB_TRY((launch_rows<false, EpiRA>(in, lda, packed + ln.w_off, ln.Kp, pb.Mp, ln.Np, ln.Kp, epi, mm_flops(pb.M, ln), s)));
  }
  return RNB_OK;
}

// FB: the forward sweep's backward.  Head: zb_{nh-1} = (fbar Wf + sbar/scale w_sdf) * D + zR, then layers nh-1 .. 1.
int layers_fb(const Layout& L, const float* packed, PointBufs& pb, bool with_feat, hipStream_t s) {
  const int64_t M = pb.M, Mp = pb.Mp;
  EpiFB epi{pb.D[L.nh - 1], pb.zR[L.nh - 1], pb.zb[L.nh - 1], L.Hp, L.hid[L.nh - 1].N, pb.sbar,
            packed + L.wsdf_off, 1.f / L.sdf_scale};
  const int K = with_feat ? L.feat.Np : 0;   // no_albedo: fbar == 0, the GEMM degenerates to its epilogue
  RNB_TRY((launch_rows<true, EpiFB>(pb.cinb, L.Cinp, packed + L.feat.w_off, L.feat.Kp, Mp, L.feat.Kp, K, epi,
                                    with_feat ? mm_flops(M, L.feat) : 0.0, s)));
  for (int l = L.nh - 1; l >= 1; --l) {
    const Lin& ln = L.hid[l];
    const Lin& lp = L.hid[l - 1];
    EpiFB epi{pb.D[l - 1], pb.zR[l - 1], pb.zb[l - 1], L.Hp, lp.N, nullptr, nullptr, 1.f};
    RNB_TRY((launch_rows<true, EpiFB>(pb.zb[l], L.Hp, packed + ln.w_off, ln.Kp, Mp, ln.Kp, ln.Np, epi, mm_flops(M, ln), s)));
  }
  return RNB_OK;
}

// ebar = d loss / d e after an SDF backward: two products in the shape of the R sweep's last steps (zb W against the
// row-major W: k-contiguous in the layer's output width).  Needs zb_0, zb_skip; the backward has flushed, so geb is free
// and becomes ebar.
int launch_sdf_ebar(const Layout& L, const float* packed, PointBufs& pb, float** ebar_out, hipStream_t s) {
  float* ebar = pb.geb;
  if (L.skip >= 1) {
    const Lin& ln = L.hid[L.skip];
    EpiSkipPE epi{ebar, L.Ep, ln.K - L.pe, L.pe};
    RNB_TRY((launch_rows<true, EpiSkipPE>(pb.zb[L.skip], L.Hp, packed + ln.w_off, ln.Kp, pb.Mp, ln.Kp, ln.Np, epi,
                                          mm_flops(pb.M, ln), s, false, nullptr, nullptr, 0, "input_adjoint")));
  }
  {
    const Lin& ln = L.hid[0];
    EpiR0 epi{ebar, L.Ep, L.pe, L.skip >= 1 ? 1 : 0};
    RNB_TRY((launch_rows<true, EpiR0>(pb.zb[0], L.Hp, packed + ln.w_off, ln.Kp, pb.Mp, ln.Kp, ln.Np, epi, mm_flops(pb.M, ln), s,
                                      false, nullptr, nullptr, 0, "input_adjoint")));
  }
  *ebar_out = ebar;
  return RNB_OK;
}

}  // namespace rnb
