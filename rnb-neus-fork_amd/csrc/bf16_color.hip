// RNB_VARIANT_BF16: the albedo network's forward and backward in bf16, used where it has the shipped shape
// (bf16_color_supported); its hidden-layer weight gradients are jobs of bf16_dw.hip.  See bf16_common.hip.h.
#include "bf16_common.hip.h"
#include "pe.hip.h"

namespace rnb {

// ---------------------------------------------------------------------------------------------------------------
// albedo network (RenderingNetwork, mode no_view_dir: models/fields.py:177-215) in bf16
// ---------------------------------------------------------------------------------------------------------------
// Input [feature | pe(p) | pe(n) | 0] (Cinp = 320 columns, the packed column order of weightnorm.hip), nc hidden ReLU
// layers of width 256, output layer (<= 4 rows, sigmoid) on the VALU with fp32 weights.  Saved for the backward in K8
// bf16: cin8 (all Cinp columns), ac8[l].  One 64-point tile per workgroup, 4 waves of 64 rows x 64 columns.
constexpr int CP = 328;    // LDS pitch (bf16 elements) of a [point][Cinp <= 320] row: 656 bytes, conflict-free ds_read_b128
constexpr int CMAX = 320;

struct BfColArgs {
  const float* pts;        // [M,3]
  const float* nrm;        // [Mp,4]
  int64_t M;
  const float* packed;
  const bfraw* wbf;
  int nc, F, pev, multires_view, Cinp, Co, squeeze;
  int Kp[RNB_MAX_LIN];
  long long w_off[RNB_MAX_LIN], wT_off[RNB_MAX_LIN], b_off[RNB_MAX_LIN];
  long long wo_off, bo_off;
  int ldwo;
  bfraw* cin8;             // [Mp,Cinp] K8: features written by the F sweep; this kernel adds the pe columns
  bfraw* ac8[RNB_MAX_LIN]; // [Mp,256] K8
  float* alb;              // [Mp,4]
  // backward
  const float* albbar;     // [Mp,4]
  bfraw* zc8[RNB_MAX_LIN]; // [Mp,256] K8
  bfraw* fbar8;            // [Mp,256] K8 (out): adjoint of the feature columns
  float* cinb;             // [Mp,Cinp] fp32 row-major: only the pe columns F.. are written (consumed by nbar_geb_kernel)
};

__global__ __launch_bounds__(256, 2) void bf_color_fwd_kernel(BfColArgs g) {
  __shared__ __attribute__((aligned(16))) bfraw X[BT * CP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int64_t row0 = (int64_t)blockIdx.x * BT;
  const int n0 = wave * 64;
  const int h = lane >> 5, cl = lane & 31;
  // features: K8 units of cin8 -> LDS rows
  {
    const bfraw* src = g.cin8 + (size_t)(row0 >> 3) * g.Cinp * 8;
    for (int u = tid; u < (BT / 8) * g.F; u += 256) {
      const int blk = u / g.F, c = u - blk * g.F;
      lds_scatter8<CP>(X, blk, c, *reinterpret_cast<const vu4*>(src + ((size_t)blk * g.Cinp + c) * 8));
    }
  }
  // pe(p), pe(n) (fp32 math, models/embedder.py:40-46): 4 threads per point = (which vector, even / odd octaves)
  {
    const int p = tid & 63, part = tid >> 6, which = part >> 1, sub = part & 1;
    const int64_t row = row0 + p;
    float v[3] = {0.f, 0.f, 0.f};
    if (row < g.M) {
      if (which == 0) { v[0] = g.pts[row * 3]; v[1] = g.pts[row * 3 + 1]; v[2] = g.pts[row * 3 + 2]; }
      else { v[0] = g.nrm[row * 4]; v[1] = g.nrm[row * 4 + 1]; v[2] = g.nrm[row * 4 + 2]; }
    }
    bfraw* xr = X + p * CP + g.F + which * g.pev;
    if (sub == 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) xr[d] = to_bf(v[d]);
      if (which == 1)
        for (int c = g.F + 2 * g.pev; c < g.Cinp; ++c) X[p * CP + c] = 0;
    }
    pe_sincos(v, g.multires_view, sub, 2, [&](int c, float sn, float co) {
      xr[c] = to_bf(sn);
      xr[c + 3] = to_bf(co);
    });
  }
  __syncthreads();
  // the pe columns of the input in K8 (Y operand of layer 0's weight gradient)
  {
    const int W = g.Cinp - g.F;
    for (int u = tid; u < (BT / 8) * W; u += 256) {
      const int blk = u / W, c = g.F + (u - blk * W);
      *reinterpret_cast<vu4*>(g.cin8 + (((size_t)(row0 >> 3) + blk) * g.Cinp + c) * 8) = lds_gather8<CP>(X, blk, c);
    }
  }
  v16f acc[2][2];
  for (int l = 0; l < g.nc; ++l) {
    bf_layer_mma<2, CP>(X, g.wbf + g.w_off[l], g.Kp[l], n0, lane, acc);
    lds_barrier();
    const float* bias = g.packed + g.b_off[l];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = n0 + tj * 32 + cl;
      const float bc = bias[col];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float a[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            a[j] = relu_nan(acc[ti][tj][4 * q + j] + bc);
            X[(ti * 32 + 8 * q + 4 * h + j) * CP + col] = to_bf(a[j]);
          }
          k8_store_quad(g.ac8[l], row0, ti, q, col, h, a[0], a[1], a[2], a[3]);
        }
    }
    lds_barrier();
  }
  // output layer + sigmoid: fp32 weights on the bf16 activations, 16 rows per wave
  {
    float w[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int u = 0; u < 4; ++u) w[c][u] = c < g.Co ? g.packed[g.wo_off + (long long)c * g.ldwo + lane + 64 * u] : 0.f;
    for (int rr = 0; rr < BT / 4; ++rr) {
      const int row = wave * (BT / 4) + rr;
      float sc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float a = bf_f(X[row * CP + lane + 64 * u]);
#pragma unroll
        for (int c = 0; c < 4; ++c) sc[c] = fmaf(a, w[c][u], sc[c]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sc[c] += __shfl_xor(sc[c], o, 64);
      if (lane < 4) {
        float v = 0.f;
        if (lane < g.Co) {
          v = sc[lane] + g.packed[g.bo_off + lane];
          if (g.squeeze) v = 1.f / (1.f + expf(-v));
        }
        g.alb[(row0 + row) * 4 + lane] = v;
      }
    }
  }
}

// backward: zo = albbar * alb (1 - alb); zc_last = (zo Wo) * relu'; zc_{l-1} = (zc_l W_l) * relu'; cinb = zc_0 W_0
__global__ __launch_bounds__(256, 2) void bf_color_bwd_kernel(BfColArgs g) {
  __shared__ __attribute__((aligned(16))) bfraw X[BT * BP];
  __shared__ float ZO[BT * 4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int64_t row0 = (int64_t)blockIdx.x * BT;
  const int n0 = wave * 64;
  const int h = lane >> 5, cl = lane & 31;
  if (tid < BT) {
    const int64_t row = row0 + tid;
    const vf4 a4 = *reinterpret_cast<const vf4*>(g.alb + row * 4);
    const vf4 g4 = *reinterpret_cast<const vf4*>(g.albbar + row * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      ZO[tid * 4 + c] = (c < g.Co && row < g.M) ? g4[c] * (g.squeeze ? a4[c] * (1.f - a4[c]) : 1.f) : 0.f;
  }
  __syncthreads();
  {   // zc_{nc-1}: one K8 unit (8 points of one column) per thread and step
    const int L = g.nc - 1;
    const bfraw* ac = g.ac8[L] + (size_t)(row0 >> 3) * FH * 8;
    bfraw* zc = g.zc8[L] + (size_t)(row0 >> 3) * FH * 8;
    for (int u = tid; u < (BT / 8) * FH; u += 256) {
      const int blk = u / FH, c = u - blk * FH;
      float w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = k < g.Co ? g.packed[g.wo_off + (long long)k * g.ldwo + c] : 0.f;
      const vu4 a = *reinterpret_cast<const vu4*>(ac + (size_t)u * 8);
      const unsigned aw[4] = {a.x, a.y, a.z, a.w};
      float z[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float av = (j & 1) ? bf_hi(aw[j >> 1]) : bf_lo(aw[j >> 1]);
        const float* zo = ZO + (blk * 8 + j) * 4;
        const float t = fmaf(zo[0], w[0], fmaf(zo[1], w[1], fmaf(zo[2], w[2], zo[3] * w[3])));
        z[j] = av > 0.f ? t : 0.f;
        X[(blk * 8 + j) * BP + c] = to_bf(z[j]);
      }
      *reinterpret_cast<vu4*>(zc + (size_t)u * 8) = vu4{pack2(z[0], z[1]), pack2(z[2], z[3]), pack2(z[4], z[5]), pack2(z[6], z[7])};
    }
  }
  __syncthreads();
  v16f acc[2][2];
  AuxBf<2> aA;
  for (int l = g.nc - 1; l >= 1; --l) {
    k8_prefetch<2>(g.ac8[l - 1], row0, n0, lane, aA);
    bf_layer_mma<2>(X, g.wbf + g.wT_off[l], FH, n0, lane, acc);   // zc_l W_l  (columns = inputs of layer l)
    lds_barrier();
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = n0 + tj * 32 + cl;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float z[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            z[j] = aux_at(aA, ti, tj, 4 * q + j) > 0.f ? acc[ti][tj][4 * q + j] : 0.f;
            X[(ti * 32 + 8 * q + 4 * h + j) * BP + col] = to_bf(z[j]);
          }
          k8_store_quad(g.zc8[l - 1], row0, ti, q, col, h, z[0], z[1], z[2], z[3]);
        }
    }
    lds_barrier();
  }
  // cinb = zc_0 W_0: columns 0 .. F-1 (features) -> fbar8 (K8 bf16, what the FB sweep and the feature head's dW read);
  // columns F .. Cin-1 (pe(p) | pe(n)) -> fp32 row-major cinb (the normal's adjoint, nbar_geb_kernel)
  bf_layer_mma<2>(X, g.wbf + g.wT_off[0], FH, n0, lane, acc);
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const int col = n0 + tj * 32 + cl;
    if (col < g.F) {
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          k8_store_quad(g.fbar8, row0, ti, q, col, h, acc[ti][tj][4 * q], acc[ti][tj][4 * q + 1], acc[ti][tj][4 * q + 2],
                        acc[ti][tj][4 * q + 3]);
    }
  }
  if (wave == 0) {   // the 64 pe columns: one more 64 x 64 block
    bf_layer_mma<2>(X, g.wbf + g.wT_off[0], FH, g.F, lane, acc);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = g.F + tj * 32 + cl;
      if (col < g.Cinp) {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            g.cinb[(size_t)(row0 + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * g.Cinp + col] = acc[ti][tj][r];
      }
    }
  }
}

// gradient of the albedo output layer: dWo[c][k] += sum_rows zo[row][c] ac_last[row][k], dbo[c] += sum_rows zo[row][c].
// One thread per column k and point slab (one slab in the deterministic variant).
__global__ __launch_bounds__(1024) void bf_color_out_bwd_kernel(const bfraw* __restrict__ ac, const float* __restrict__ alb,
                                                                const float* __restrict__ albbar, int Co, int squeeze,
                                                                int64_t M, int64_t rows_per_blk, int ldwo,
                                                                float* __restrict__ dWo, float* __restrict__ dbo) {
  __shared__ double red[4][4][FH], redb[4][4];
  const int c = threadIdx.x & 255, ph = threadIdx.x >> 8;   // column, one of 4 row phases
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk;
  const int64_t r1 = r0 + rows_per_blk < M ? r0 + rows_per_blk : M;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = r0 + 8 * ph; r < r1; r += 32) {
    const vu4 av = *reinterpret_cast<const vu4*>(ac + ((size_t)(r >> 3) * FH + c) * 8);
    const unsigned aw[4] = {av.x, av.y, av.z, av.w};
    float t[4] = {0.f, 0.f, 0.f, 0.f}, tb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (r + j < r1) {
        const float a = (j & 1) ? bf_hi(aw[j >> 1]) : bf_lo(aw[j >> 1]);
        const vf4 a4 = *reinterpret_cast<const vf4*>(alb + (r + j) * 4);
        const vf4 g4 = *reinterpret_cast<const vf4*>(albbar + (r + j) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float zo = k < Co ? g4[k] * (squeeze ? a4[k] * (1.f - a4[k]) : 1.f) : 0.f;
          t[k] = fmaf(zo, a, t[k]);
          tb[k] += zo;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { s[k] += (double)t[k]; sb[k] += (double)tb[k]; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    red[ph][k][c] = s[k];
    if (c == 0) redb[ph][k] = sb[k];
  }
  __syncthreads();
  if (ph == 0) {
    for (int k = 0; k < Co; ++k) {
      atomicAdd(dWo + (size_t)k * ldwo + c, (float)(red[0][k][c] + red[1][k][c] + red[2][k][c] + red[3][k][c]));
      if (c == 0) atomicAdd(dbo + k, (float)(redb[0][k] + redb[1][k] + redb[2][k] + redb[3][k]));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// the albedo network runs in bf16 too when it has the shipped shape; otherwise its fp32 kernels (layers.hip) are used
bool bf16_color_supported(const Layout& L) {
  if (L.F != FH || L.Hc != FH || L.Hcp != FH) return false;
  if (L.Cinp > CMAX || L.Cinp % 64 != 0 || L.Cinp - L.F > 64) return false;
  if (L.nc < 1 || L.Co < 1 || L.Co > 4) return false;
  return true;
}

static void fill_col(const Layout& L, const float* packed, const float* pts, PointBufs& pb, BfColArgs& g) {
  memset(&g, 0, sizeof(g));
  g.pts = pts;
  g.nrm = pb.nrm;
  g.M = pb.M;
  g.packed = packed;
  g.wbf = reinterpret_cast<const bfraw*>(packed + L.total);
  g.nc = L.nc; g.F = L.F; g.pev = L.pev; g.multires_view = L.multires_view; g.Cinp = L.Cinp; g.Co = L.Co;
  g.squeeze = L.squeeze;
  for (int l = 0; l < L.nc; ++l) {
    g.Kp[l] = L.col[l].Kp;
    g.w_off[l] = L.col[l].w_off;
    g.wT_off[l] = L.col[l].wT_off;
    g.b_off[l] = L.col[l].b_off;
    g.ac8[l] = reinterpret_cast<bfraw*>(pb.ac8[l]);
    g.zc8[l] = reinterpret_cast<bfraw*>(pb.zc8[l]);
  }
  g.wo_off = L.colo.w_off;
  g.bo_off = L.colo.b_off;
  g.ldwo = L.colo.Kp;
  g.cin8 = reinterpret_cast<bfraw*>(pb.cin8);
  g.alb = pb.alb;
  g.albbar = pb.albbar;
  g.fbar8 = reinterpret_cast<bfraw*>(pb.fbar_k8);
  g.cinb = pb.cinb;
}

static double color_flops(const Layout& L, int64_t M, int first) {
  double fl = 0;
  for (int l = first; l < L.nc; ++l) fl += 2.0 * (double)M * L.col[l].N * L.col[l].K;
  return fl;
}

// C: albedo network forward on the tile state the F and R sweeps left (cin8 features, pb.nrm)
int bf16_color_forward(const Layout& L, const float* packed, PointBufs& pb, const float* pts, hipStream_t s) {
  BfColArgs g;
  fill_col(L, packed, pts, pb, g);
  ProfScope prof(color_flops(L, pb.M, 0) + 2.0 * (double)pb.M * L.colo.N * L.colo.K, s, "albedo_fwd");
  hipLaunchKernelGGL(bf_color_fwd_kernel, dim3((unsigned)(pb.Mp / BT)), dim3(256), 0, s, g);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// C': albedo network backward (writes zc8, fbar8, the pe columns of cinb, dWo / dbo); its hidden-layer weight
// gradients are jobs of bf16_dw_backward's grouped launch
int bf16_color_backward(const Layout& L, const float* packed, PointBufs& pb, float* packed_grad, hipStream_t s) {
  BfColArgs g;
  fill_col(L, packed, nullptr, pb, g);
  {
    ProfScope prof(color_flops(L, pb.M, 0) + 2.0 * (double)pb.M * L.colo.N * L.colo.K, s, "albedo_bwd");
    hipLaunchKernelGGL(bf_color_bwd_kernel, dim3((unsigned)(pb.Mp / BT)), dim3(256), 0, s, g);
    RNB_CHECK_LAUNCH();
  }
  const int64_t rows_per_blk = bf_rows_per_slab(L, pb.M);
  hipLaunchKernelGGL(bf_color_out_bwd_kernel, dim3((unsigned)((pb.M + rows_per_blk - 1) / rows_per_blk)), dim3(1024), 0, s,
                     reinterpret_cast<const bfraw*>(pb.ac8[L.nc - 1]), pb.alb, pb.albbar, L.Co, L.squeeze, pb.M, rows_per_blk,
                     L.colo.Kp, packed_grad + L.colo.w_off, packed_grad + L.colo.b_off);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

}  // namespace rnb
