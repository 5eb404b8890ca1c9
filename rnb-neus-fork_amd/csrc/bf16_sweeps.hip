// RNB_VARIANT_BF16: the four sweeps of the SDF network (F, R, RA, FB) and the packer of the bf16 weight mirror.  The route,
// its number formats and the K8 layout of the saved state are described in bf16_common.hip.h.
#include "bf16_common.hip.h"
#include "pe.hip.h"

namespace rnb {

// ---------------------------------------------------------------------------------------------------------------
// F sweep
// ---------------------------------------------------------------------------------------------------------------
struct BfFwdArgs {
  const float* pts;        // [M,3]
  int64_t M;
  const float* packed;     // fp32 packed weights (biases, sdf head row)
  const bfraw* wbf;        // bf16 mirror of the packed buffer (same offsets)
  SdfNetArgs net;
  int with_feat;
  float* cin;              // [Mp,Cinp] fp32 feature block destination (with_feat, cin8 == nullptr)
  bfraw* cin8;             // [Mp,Cinp] K8 bf16 feature block destination (bf16 albedo path) or nullptr
  float* sdf;              // [Mp]
  float* x4;               // [Mp,4]            (SAVE)
  bfraw* e;                // [Mp,64]  K8       (SAVE) positional encoding = input of layer 0
  bfraw* a[RNB_MAX_LIN];   // [Mp,256] K8       (SAVE)
  bfraw* D[RNB_MAX_LIN];   // [Mp,256] K8       (SAVE)
  GridGen grid;
};

template <bool SAVE, int TI>
__global__ __launch_bounds__(BfCfg<TI>::NT, TI == 1 ? 4 : 2) void bf_forward_kernel(BfFwdArgs g) {
  constexpr int NW = BfCfg<TI>::NW, NT = BfCfg<TI>::NT;
  __shared__ __attribute__((aligned(16))) bfraw X[BT * BP];
  __shared__ float E[BT * FEP];     // fp32 copy of the positional encoding for the skip connection
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int64_t row0 = (int64_t)blockIdx.x * BT;
  const int n0 = (wave & 3) * 64;          // column group of the wave
  const int rb = (wave >> 2) * 32;         // first row of the wave inside the tile (TI == 1: two row halves)
  const int64_t rowW = row0 + rb;
  const bfraw* Xw = X + rb * BP;
  const int h = lane >> 5, cl = lane & 31;

  // ---- positional encoding of the tile (fp32 math, models/embedder.py:40-46) ---------------------------------
  {
    constexpr int PARTS = NT / BT;   // 4 or 8 threads per point
    const int p = tid % BT, part = tid / BT;
    const int64_t row = row0 + p;
    float x[3];
    sweep_point(g.grid, g.pts, row, g.M, g.net.scale, x);
    bfraw* xr = X + p * BP;
    float* er = E + p * FEP;
    if (part == 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) { xr[d] = to_bf(x[d]); er[d] = x[d]; }
      for (int c = g.net.pe; c < g.net.Ep; ++c) xr[c] = 0;
      if (SAVE) {
        g.x4[row * 4] = x[0]; g.x4[row * 4 + 1] = x[1]; g.x4[row * 4 + 2] = x[2]; g.x4[row * 4 + 3] = 0.f;
      }
    }
    pe_sincos(x, g.net.multires, part, PARTS, [&](int c, float s, float co) {
      xr[c] = to_bf(s); xr[c + 3] = to_bf(co);
      er[c] = s; er[c + 3] = co;
    });
  }
  __syncthreads();
  if (SAVE) {   // e (bf16, K8, 64 columns): the Y operand of layer 0's weight gradient
    for (int u = tid; u < (BT / 8) * g.net.Ep; u += NT) {
      const int blk = u / g.net.Ep, c = u - blk * g.net.Ep;
      *reinterpret_cast<vu4*>(g.e + (((size_t)(row0 >> 3) + blk) * g.net.Ep + c) * 8) = lds_gather8<BP>(X, blk, c);
    }
  }

  v16f acc[TI][2];
  // cross-layer weight prefetch: the next product's block 0 is in flight during a layer's epilogue
  BfMma<TI> mm;
  mm.request(g.wbf + g.net.w_off[0], g.net.Kp[0], n0, lane);
  for (int l = 0; l < g.net.nh; ++l) {
    const bfraw* wn = l + 1 < g.net.nh ? g.wbf + g.net.w_off[l + 1] : (g.with_feat ? g.wbf + g.net.wf_off : nullptr);
    if (l == 0) mm.template run<64>(Xw, g.wbf + g.net.w_off[0], n0, lane, acc, wn, FH, n0);   // (fused_supported: Ep = 64, hidden 256)
    else mm.template run<256>(Xw, g.wbf + g.net.w_off[l], n0, lane, acc, wn, FH, n0);
    lds_barrier();   // every wave has finished reading the input activations (the tile is updated in place)
    const int lo = opaque(lane), h = lo >> 5, cl = lo & 31;
    const float* bias = g.packed + g.net.b_off[l];
    const int n_real = g.net.n_real[l];
    const bool pe_tail = (l + 1 == g.net.skip);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = n0 + tj * 32 + cl;
      const float bc = bias[col];
      const bool tile_full = n0 + tj * 32 + 32 <= n_real;   // wave-uniform: no per-element column tests
      const bool real = col < n_real;
      const bool pe_col = pe_tail && !real && col < n_real + g.net.pe;
#pragma unroll
      for (int ti = 0; ti < TI; ++ti) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float a[4], D[4];
          if (tile_full) {
#pragma unroll
            for (int j = 0; j < 4; ++j) softplus_aD_fast(acc[ti][tj][4 * q + j] + bc, a[j], D[j]);
          } else {   // only the tile straddling the skip connection's PE columns
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (real) softplus_aD_fast(acc[ti][tj][4 * q + j] + bc, a[j], D[j]);
              else { a[j] = pe_col ? E[(rb + 4 * h) * FEP + (col - n_real) + (ti * 32 + 8 * q + j) * FEP] : 0.f; D[j] = 0.f; }
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) X[(rb + 4 * h) * BP + col + (ti * 32 + 8 * q + j) * BP] = to_bf(a[j]);
          if (SAVE) {
            k8_store_quad(g.a[l], rowW, ti, q, col, h, a[0], a[1], a[2], a[3]);
            k8_store_quad(g.D[l], rowW, ti, q, col, h, D[0], D[1], D[2], D[3]);
          }
        }
      }
    }
    lds_barrier();   // the new activations are visible to every wave
  }

  // ---- sdf head: row 0 of the output layer, fp32 weights on the bf16 activations ---------------------------------
  {
    const float* ws = g.packed + g.net.wsdf_off;
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = ws[lane + 64 * u];
    const float bs = g.packed[g.net.bsdf_off];
    for (int rr = 0; rr < BT / NW; ++rr) {
      const int row = wave * (BT / NW) + rr;
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) s = fmaf(bf_f(X[row * BP + lane + 64 * u]), w[u], s);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) {
        const float v = (s + bs) / g.net.scale;
        sweep_store_sdf(g.grid, g.sdf, row0, row, g.M, v);
      }
    }
  }
  // ---- feature head: rows 1.. of the output layer, written (fp32) into the albedo network's input -------------------
  if (g.with_feat) {
    mm.template run<256>(Xw, g.wbf + g.net.wf_off, n0, lane, acc, nullptr, 0, 0);   // (block 0 was requested by the last hidden layer)
    const float* bias = g.packed + g.net.bf_off;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = n0 + tj * 32 + cl;
      if (col < g.net.F) {
        const float bc = bias[col];
        if (g.cin8 != nullptr) {
#pragma unroll
          for (int ti = 0; ti < TI; ++ti)
#pragma unroll
            for (int q = 0; q < 4; ++q)
              k8_store_quad(g.cin8, rowW, ti, q, col, h, acc[ti][tj][4 * q] + bc, acc[ti][tj][4 * q + 1] + bc,
                            acc[ti][tj][4 * q + 2] + bc, acc[ti][tj][4 * q + 3] + bc, g.net.Cinp);
        } else {
#pragma unroll
          for (int ti = 0; ti < TI; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = rb + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
              g.cin[(size_t)(row0 + row) * g.net.Cinp + col] = acc[ti][tj][r] + bc;
            }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward-shaped sweeps
// ---------------------------------------------------------------------------------------------------------------
struct BfBwdArgs {
  const float* packed;
  const bfraw* wbf;
  int64_t M;
  SdfNetArgs net;
  bfraw* D[RNB_MAX_LIN];
  bfraw* gz[RNB_MAX_LIN];
  bfraw* u[RNB_MAX_LIN + 1];   // u[0]: [Mp,64] K8 (written by RA from geb); u[l >= 1]: [Mp,256] K8
  bfraw* zR[RNB_MAX_LIN];
  bfraw* zb[RNB_MAX_LIN];
  bfraw* fbar8;         // [Mp,256] K8: the feature part of the albedo net's input adjoint (written by FB)
  const float* x4;      // [Mp,4]
  float* nrm;           // [Mp,4]      (R)
  const float* geb;     // [Mp,Ep] fp32 row-major (RA)
  const float* sbar;    // [Mp]        (FB)
  const float* fbar;    // [Mp,ld_fbar] fp32 row-major, first 256 columns, or nullptr (FB; fp32 albedo path)
  int ld_fbar;
  int fbar_in_k8;       // 1: fbar8 already holds the feature adjoint (bf16 albedo path), read it instead of `fbar`
};

// R: gz_l = g_l * D_l, g_{l-1} = gz_l W_l, normal = J_pe^T g_e
template <int TI>
__global__ __launch_bounds__(BfCfg<TI>::NT, TI == 1 ? 4 : 2) void bf_reverse_kernel(BfBwdArgs g) {
  constexpr int NT = BfCfg<TI>::NT;
  __shared__ __attribute__((aligned(16))) bfraw X[BT * BP];
  __shared__ float GE[BT * FEP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int64_t row0 = (int64_t)blockIdx.x * BT;
  const int n0 = (wave & 3) * 64;          // column group of the wave
  const int rb = (wave >> 2) * 32;         // first row of the wave inside the tile (TI == 1: two row halves)
  const int64_t rowW = row0 + rb;
  const bfraw* Xw = X + rb * BP;
  const int h = lane >> 5, cl = lane & 31;

  // seed: gz_{nh-1} = w_sdf * D_{nh-1}; one K8 unit (8 points of one column) per thread and step
  {
    const bfraw* Dl = g.D[g.net.nh - 1] + (size_t)(row0 >> 3) * FH * 8;
    bfraw* gzl = g.gz[g.net.nh - 1] + (size_t)(row0 >> 3) * FH * 8;
    const float* ws = g.packed + g.net.wsdf_off;
    for (int u = tid; u < (BT / 8) * FH; u += NT) {
      const int blk = u / FH, c = u - blk * FH;
      const vu4 d = *reinterpret_cast<const vu4*>(Dl + (size_t)u * 8);
      const float w = ws[c];
      const float v[8] = {bf_lo(d.x) * w, bf_hi(d.x) * w, bf_lo(d.y) * w, bf_hi(d.y) * w,
                          bf_lo(d.z) * w, bf_hi(d.z) * w, bf_lo(d.w) * w, bf_hi(d.w) * w};
      const vu4 o = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
      *reinterpret_cast<vu4*>(gzl + (size_t)u * 8) = o;
#pragma unroll
      for (int j = 0; j < 8; ++j) X[(blk * 8 + j) * BP + c] = to_bf(v[j]);
    }
    for (int idx = tid; idx < BT * FEP; idx += NT) GE[idx] = 0.f;
  }
  __syncthreads();

  v16f acc[TI][2];
  AuxBf<TI> aD;
  BfMma<TI> mm;
  mm.request(g.wbf + g.net.wT_off[g.net.nh - 1], FH, n0, lane);
  for (int l = g.net.nh - 1; l >= 1; --l) {
    k8_prefetch<TI>(g.D[l - 1], rowW, n0, opaque(lane), aD);
    const bfraw* wn = (l > 1 || n0 < 64) ? g.wbf + g.net.wT_off[l - 1] : nullptr;   // layer 0's product: wave(s) of columns 0..63
    mm.template run<256>(Xw, g.wbf + g.net.wT_off[l], n0, lane, acc, wn, FH, n0);   // g = gz_l W_l  (columns = inputs of layer l)
    lds_barrier();
    const int lo = opaque(lane), h = lo >> 5, cl = lo & 31;
    const bool is_skip = (l == g.net.skip);
    const int ksplit = is_skip ? FH - g.net.pe : FH;   // columns that belong to layer l-1's output
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = n0 + tj * 32 + cl;
      const bool tile_full = n0 + tj * 32 + 32 <= ksplit;   // wave-uniform: no per-element column tests
#pragma unroll
      for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float o[4];
          if (tile_full) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = acc[ti][tj][4 * q + j] * aux_at(aD, ti, tj, 4 * q + j);
          } else {   // only the tile straddling the skip connection's PE columns
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = 4 * q + j;
              const float v = acc[ti][tj][r];
              if (col < ksplit) o[j] = v * aux_at(aD, ti, tj, r);
              else {
                if (col < ksplit + g.net.pe) GE[(rb + 4 * h) * FEP + (col - ksplit) + (ti * 32 + 8 * q + j) * FEP] = v;   // skip connection: straight to g_e
                o[j] = 0.f;
              }
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) X[(rb + 4 * h) * BP + col + (ti * 32 + 8 * q + j) * BP] = to_bf(o[j]);
          k8_store_quad(g.gz[l - 1], rowW, ti, q, col, h, o[0], o[1], o[2], o[3]);
        }
    }
    lds_barrier();
  }
  // layer 0: g_e += gz_0 W_0 (Ep = 64 columns: wave 0)
  if (n0 < 64) {
    if (g.net.nh == 1) mm.request(g.wbf + g.net.wT_off[0], FH, n0, lane);
    mm.template run<256>(Xw, g.wbf + g.net.wT_off[0], n0, lane, acc, nullptr, 0, 0);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = n0 + tj * 32 + cl;
      if (col < g.net.pe) {
#pragma unroll
        for (int ti = 0; ti < TI; ++ti)
#pragma unroll
          for (int r = 0; r < 16; ++r) GE[(rb + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * FEP + col] += acc[ti][tj][r];
      }
    }
  }
  __syncthreads();
  if (tid < BT) {   // normal = J_pe(x)^T g_e  (fp32)
    const int64_t row = row0 + tid;
    const float* ge = GE + tid * FEP;
    float n[3] = {ge[0], ge[1], ge[2]};
    pe_adjoint(g.x4 + row * 4, ge, g.net.multires, 0, 1, n);
    g.nrm[row * 4] = n[0]; g.nrm[row * 4 + 1] = n[1]; g.nrm[row * 4 + 2] = n[2]; g.nrm[row * 4 + 3] = 0.f;
  }
}

// RA: u_{l+1} = (u_l W_l^T) * D_l, zR_l = 100 (u_l W_l^T) gz_l (1 - D_l)
template <int TI>
__global__ __launch_bounds__(BfCfg<TI>::NT, TI == 1 ? 4 : 2) void bf_ra_kernel(BfBwdArgs g) {
  constexpr int NT = BfCfg<TI>::NT;
  __shared__ __attribute__((aligned(16))) bfraw X[BT * BP];
  __shared__ float E[BT * FEP];   // adjoint of g_e of the tile (re-enters at the skip connection)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int64_t row0 = (int64_t)blockIdx.x * BT;
  const int n0 = (wave & 3) * 64;          // column group of the wave
  const int rb = (wave >> 2) * 32;         // first row of the wave inside the tile (TI == 1: two row halves)
  const int64_t rowW = row0 + rb;
  const bfraw* Xw = X + rb * BP;

  for (int idx = tid; idx < BT * g.net.Ep; idx += NT) {
    const int r = idx / g.net.Ep, c = idx - r * g.net.Ep;
    const float v = g.geb[(row0 + r) * g.net.Ep + c];
    X[r * BP + c] = to_bf(v);
    if (c < FEP) E[r * FEP + c] = v;
  }
  __syncthreads();
  // u_0 in K8 (the Y operand of layer 0's weight gradient)
  for (int u = tid; u < (BT / 8) * g.net.Ep; u += NT) {
    const int blk = u / g.net.Ep, c = u - blk * g.net.Ep;
    *reinterpret_cast<vu4*>(g.u[0] + (((size_t)(row0 >> 3) + blk) * g.net.Ep + c) * 8) = lds_gather8<BP>(X, blk, c);
  }

  v16f acc[TI][2];
  AuxBf<TI> aD, aG;
  // no cross-layer weight prefetch and 32-k weight blocks here: the two epilogue operand tiles already fill the registers
  BfMma<TI> mm;
  mm.request(g.wbf + g.net.w_off[0], g.net.Kp[0], n0, lane);
  for (int l = 0; l < g.net.nh; ++l) {
    const int lp = opaque(lane);
    k8_prefetch<TI>(g.D[l], rowW, n0, lp, aD);
    k8_prefetch<TI>(g.gz[l], rowW, n0, lp, aG);
    const bfraw* wn = l + 1 < g.net.nh ? g.wbf + g.net.w_off[l + 1] : nullptr;
    if (l == 0) mm.template run<64>(Xw, g.wbf + g.net.w_off[0], n0, lane, acc, wn, FH, n0);   // gzb = u_l W_l^T
    else mm.template run<256>(Xw, g.wbf + g.net.w_off[l], n0, lane, acc, wn, FH, n0);
    lds_barrier();
    const int lo = opaque(lane), h = lo >> 5, cl = lo & 31;
    const int n_real = g.net.n_real[l];
    const bool pe_tail = (l + 1 == g.net.skip);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = n0 + tj * 32 + cl;
      const bool tile_full = n0 + tj * 32 + 32 <= n_real;   // wave-uniform: no per-element column tests
#pragma unroll
      for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float un[4], zr[4];
          if (tile_full) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = 4 * q + j;
              const float v = acc[ti][tj][r];
              un[j] = v * aux_at(aD, ti, tj, r);
              zr[j] = ((v - un[j]) * aux_at(aG, ti, tj, r)) * 100.f;
            }
          } else {   // only the tile straddling the skip connection's PE columns
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = 4 * q + j;
              const float v = acc[ti][tj][r];
              if (col < n_real) {
                un[j] = v * aux_at(aD, ti, tj, r);
                zr[j] = ((v - un[j]) * aux_at(aG, ti, tj, r)) * 100.f;
              } else {
                zr[j] = 0.f;
                un[j] = (pe_tail && col < n_real + g.net.pe) ? E[(rb + 4 * h) * FEP + (col - n_real) + (ti * 32 + 8 * q + j) * FEP] : 0.f;
              }
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) X[(rb + 4 * h) * BP + col + (ti * 32 + 8 * q + j) * BP] = to_bf(un[j]);
          k8_store_quad(g.u[l + 1], rowW, ti, q, col, h, un[0], un[1], un[2], un[3]);
          k8_store_quad(g.zR[l], rowW, ti, q, col, h, zr[0], zr[1], zr[2], zr[3]);
        }
    }
    lds_barrier();
  }
}

// FB: zb_{l-1} = (zb_l W_l) * D_{l-1} + zR_{l-1}, head: ab_{nh-1} = fbar W_feat + sbar / scale * w_sdf
template <int TI>
__global__ __launch_bounds__(BfCfg<TI>::NT, TI == 1 ? 4 : 2) void bf_fb_kernel(BfBwdArgs g) {
  constexpr int NT = BfCfg<TI>::NT;
  __shared__ __attribute__((aligned(16))) bfraw X[BT * BP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int64_t row0 = (int64_t)blockIdx.x * BT;
  const int n0 = (wave & 3) * 64;          // column group of the wave
  const int rb = (wave >> 2) * 32;         // first row of the wave inside the tile (TI == 1: two row halves)
  const int64_t rowW = row0 + rb;
  const bfraw* Xw = X + rb * BP;

  v16f acc[TI][2];
  AuxBf<TI> aD, aZ;
  BfMma<TI> mm;
  const bool has_head = g.fbar_in_k8 || g.fbar != nullptr;
  if (has_head) mm.request(g.wbf + g.net.wfT_off, FH, n0, lane);
  else if (g.net.nh > 1) mm.request(g.wbf + g.net.wT_off[g.net.nh - 1], FH, n0, lane);
  const bfraw* w_first = g.net.nh > 1 ? g.wbf + g.net.wT_off[g.net.nh - 1] : nullptr;
  bf_zero<TI>(acc);
  if (g.fbar_in_k8) {
    const bfraw* fb = g.fbar8 + (size_t)(row0 >> 3) * FH * 8;
    for (int u = tid; u < (BT / 8) * FH; u += NT)
      lds_scatter8<BP>(X, u / FH, u % FH, *reinterpret_cast<const vu4*>(fb + (size_t)u * 8));
    __syncthreads();
    mm.template run<256>(Xw, g.wbf + g.net.wfT_off, n0, lane, acc, w_first, FH, n0);
    lds_barrier();
  } else if (g.fbar != nullptr) {
    // fbar (fp32 row-major, from the albedo net's backward) -> LDS bf16, and K8 for the feature head's dW
    for (int idx = tid; idx < BT * FH / 4; idx += NT) {
      const int r = idx >> 6, c4 = idx & 63;
      const vf4 v = *reinterpret_cast<const vf4*>(g.fbar + (size_t)(row0 + r) * g.ld_fbar + c4 * 4);
      const vu2 o = {pack2(v.x, v.y), pack2(v.z, v.w)};
      *reinterpret_cast<vu2*>(X + r * BP + c4 * 4) = o;
    }
    __syncthreads();
    for (int u = tid; u < (BT / 8) * FH; u += NT) {
      const int blk = u / FH, c = u - blk * FH;
      *reinterpret_cast<vu4*>(g.fbar8 + (((size_t)(row0 >> 3) + blk) * FH + c) * 8) = lds_gather8<BP>(X, blk, c);
    }
    mm.template run<256>(Xw, g.wbf + g.net.wfT_off, n0, lane, acc, w_first, FH, n0);
    lds_barrier();
  }
  for (int l = g.net.nh - 1; l >= 0; --l) {
    const int lo = opaque(lane), h = lo >> 5, cl = lo & 31;
    k8_prefetch<TI>(g.D[l], rowW, n0, lo, aD);
    k8_prefetch<TI>(g.zR[l], rowW, n0, lo, aZ);
    const int n_real = g.net.n_real[l];
    const bool head = (l == g.net.nh - 1);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = n0 + tj * 32 + cl;
      const float ws = head ? g.packed[g.net.wsdf_off + col] : 0.f;
#pragma unroll
      for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float zb[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * q + j;
            float v = acc[ti][tj][r];
            if (head) v = fmaf(g.sbar[row0 + rb + 4 * h + (ti * 32 + 8 * q + j)] * g.net.inv_scale, ws, v);   // the sdf head's contribution
            zb[j] = col < n_real ? fmaf(v, aux_at(aD, ti, tj, r), aux_at(aZ, ti, tj, r)) : 0.f;
            X[(rb + 4 * h) * BP + col + (ti * 32 + 8 * q + j) * BP] = to_bf(zb[j]);
          }
          k8_store_quad(g.zb[l], rowW, ti, q, col, h, zb[0], zb[1], zb[2], zb[3]);
        }
    }
    if (l == 0) break;
    lds_barrier();
    mm.template run<256>(Xw, g.wbf + g.net.wT_off[l], n0, lane, acc, l > 1 ? g.wbf + g.net.wT_off[l - 1] : nullptr, FH, n0);   // ab_{l-1} = zb_l W_l
    lds_barrier();   // every wave has finished reading the tile
  }
}

// fp32 packed weights -> bf16 mirror: every matrix that serves as an MFMA B operand, at its own element offset, in
// fragment order (see bf_load_b).  One workgroup per 32-row x 16-k fragment... one thread per 16-byte unit.
struct BfPackEntry { long long off; int N, K; int unit_begin; };
constexpr int kMaxPack = 4 * RNB_MAX_LIN + 4;
struct BfPackTable { int n, total_units; BfPackEntry e[kMaxPack]; };
__global__ void bf_pack_kernel(const float* __restrict__ src, BfPackTable t, bfraw* __restrict__ dst) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= t.total_units) return;
  int ei = 0;
  while (ei + 1 < t.n && u >= t.e[ei + 1].unit_begin) ++ei;
  const BfPackEntry en = t.e[ei];
  const int lu = u - en.unit_begin;            // unit inside the matrix: fragment lu / 64, lane lu % 64
  const int frag = lu >> 6, lane = lu & 63;
  const int nks = en.K >> 4;
  const int nt = frag / nks, ks = frag - nt * nks;
  const int c = lane & 31, h = lane >> 5;
  const float* sp = src + en.off + (size_t)(nt * 32 + c) * en.K + ks * 16 + h * 8;
  const vu4 o = {pack2(sp[0], sp[1]), pack2(sp[2], sp[3]), pack2(sp[4], sp[5]), pack2(sp[6], sp[7])};
  *reinterpret_cast<vu4*>(dst + en.off + (size_t)lu * 8) = o;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int bf16_pack_weights(const Layout& L, float* packed, hipStream_t s) {
  bfraw* dst = reinterpret_cast<bfraw*>(packed + L.total);
  BfPackTable t;
  t.n = 0;
  t.total_units = 0;
  auto add = [&](long long off, int N, int K) {
    if (off < 0 || N <= 0 || K <= 0) return;
    BfPackEntry& e = t.e[t.n++];
    e.off = off; e.N = N; e.K = K; e.unit_begin = t.total_units;
    t.total_units += N * K / 8;
  };
  for (int l = 0; l < L.nh; ++l) {
    add(L.hid[l].w_off, L.hid[l].Np, L.hid[l].Kp);
    add(L.hid[l].wT_off, L.hid[l].Kp, L.hid[l].Np);
  }
  if (L.F > 0) {
    add(L.feat.w_off, L.feat.Np, L.feat.Kp);
    add(L.feat.wT_off, L.feat.Kp, L.feat.Np);
    for (int l = 0; l < L.nc; ++l) {
      add(L.col[l].w_off, L.col[l].Np, L.col[l].Kp);
      add(L.col[l].wT_off, L.col[l].Kp, L.col[l].Np);
    }
  }
  hipLaunchKernelGGL(bf_pack_kernel, dim3((unsigned)((t.total_units + 255) / 256)), dim3(256), 0, s, packed, t, dst);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// rows per wave of the sweeps: RNB_VARIANT_{FWD,BWD}_TI (1: 32 rows x 8 waves, 2: 64 rows x 4 waves).  Default 2:
// measured 4.23 ms / step against 5.04 ms with TI = 1 on both (512 rays x 256 samples) — the 8-wave form doubles the
// weight bytes each CU pulls from L2 per point (every fragment feeds one row tile instead of two), and that stream,
// not latency, is what these sweeps wait for.
static int bf_ti(const Layout& L, int shift) {
  const int v = L.knob(shift);
  return v == 1 ? 1 : 2;
}

static const bfraw* wbf_of(const Layout& L, const float* packed) { return reinterpret_cast<const bfraw*>(packed + L.total); }

// the tile height of a sweep -> f(TI as a constant, grid, block): the kernel's own workgroup shape
template <class F>
static void pick_bf_tile(int ti, const PointBufs& pb, F&& f) {
  pick_c<1, 2>(ti, [&](auto ti_c) { f(ti_c, dim3((unsigned)(pb.Mp / BT)), dim3(BfCfg<decltype(ti_c)::value>::NT)); });
}

int bf16_forward(const Layout& L, const float* packed, const float* pts, int64_t M, PointBufs& pb, bool save, bool need_feat,
                 hipStream_t s, const GridGen* grid, bool feat_k8) {
  BfFwdArgs g;
  memset(&g, 0, sizeof(g));
  g.net = sdf_net_args(L);
  if (grid) g.grid = *grid;
  g.pts = pts;
  g.M = M;
  g.packed = packed;
  g.wbf = wbf_of(L, packed);
  for (int l = 0; l < L.nh; ++l) {
    g.a[l] = reinterpret_cast<bfraw*>(pb.a[l]);
    g.D[l] = reinterpret_cast<bfraw*>(pb.D[l]);
  }
  g.with_feat = need_feat ? 1 : 0;
  g.cin = pb.cin;
  g.cin8 = feat_k8 ? reinterpret_cast<bfraw*>(pb.cin8) : nullptr;
  g.sdf = pb.sdf;
  g.x4 = pb.x;
  g.e = reinterpret_cast<bfraw*>(pb.e);
  ProfScope prof(sdf_sweep_flops(L, M, 0, true, need_feat), s, save ? "F_sweep(save)" : "F_sweep(forward_only)");
  pick_bf_tile(bf_ti(L, RNB_VARIANT_FWD_TI_SHIFT), pb, [&](auto ti_c, dim3 grid, dim3 block) {
    if (save) hipLaunchKernelGGL((bf_forward_kernel<true, decltype(ti_c)::value>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((bf_forward_kernel<false, decltype(ti_c)::value>), grid, block, 0, s, g);
  });
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

static void fill_bwd(const Layout& L, const float* packed, PointBufs& pb, BfBwdArgs& g) {
  memset(&g, 0, sizeof(g));
  g.net = sdf_net_args(L);
  g.packed = packed;
  g.wbf = wbf_of(L, packed);
  g.M = pb.M;
  for (int l = 0; l < L.nh; ++l) {
    g.D[l] = reinterpret_cast<bfraw*>(pb.D[l]);
    g.gz[l] = reinterpret_cast<bfraw*>(pb.gz[l]);
    g.zR[l] = reinterpret_cast<bfraw*>(pb.zR[l]);
    g.zb[l] = reinterpret_cast<bfraw*>(pb.zb[l]);
  }
  g.u[0] = reinterpret_cast<bfraw*>(pb.u0_k8);
  for (int l = 1; l <= L.nh; ++l) g.u[l] = reinterpret_cast<bfraw*>(pb.u[l]);
  g.fbar8 = reinterpret_cast<bfraw*>(pb.fbar_k8);
  g.x4 = pb.x;
  g.nrm = pb.nrm;
  g.geb = pb.geb;
  g.sbar = pb.sbar;
}

int bf16_reverse(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s) {
  BfBwdArgs g;
  fill_bwd(L, packed, pb, g);
  ProfScope prof(sdf_sweep_flops(L, pb.M, 0, false, false), s, "R_sweep");
  pick_bf_tile(bf_ti(L, RNB_VARIANT_BWD_TI_SHIFT), pb, [&](auto ti_c, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(bf_reverse_kernel<decltype(ti_c)::value>, grid, block, 0, s, g);
  });
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// RA: u_0 = pb.geb -> u_{l+1} and zR_l of every layer (and u_0 in K8)
int bf16_ra(const Layout& L, const float* packed, PointBufs& pb, hipStream_t s) {
  BfBwdArgs g;
  fill_bwd(L, packed, pb, g);
  ProfScope prof(sdf_sweep_flops(L, pb.M, 0, false, false), s, "RA_sweep");
  pick_bf_tile(bf_ti(L, RNB_VARIANT_BWD_TI_SHIFT), pb, [&](auto ti_c, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(bf_ra_kernel<decltype(ti_c)::value>, grid, block, 0, s, g);
  });
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// FB: zb_l of every layer from pb.sbar and, with_color, the adjoint of the feature head's output.  After the bf16 albedo
// backward that adjoint is already bf16 K8 in pb.fbar_k8 (fbar_in_k8); after the fp32 one it is the first 256 columns of
// pb.cinb's fp32 rows, which FB rounds and also leaves in pb.fbar_k8 for the feature head's weight gradient.
int bf16_fb(const Layout& L, const float* packed, PointBufs& pb, bool with_color, hipStream_t s) {
  BfBwdArgs g;
  fill_bwd(L, packed, pb, g);
  const bool color_bf16 = with_color && L.route.color == COLOR_BF16;
  g.fbar = (with_color && !color_bf16) ? pb.cinb : nullptr;
  g.ld_fbar = L.Cinp;
  g.fbar_in_k8 = color_bf16 ? 1 : 0;
  ProfScope prof(sdf_sweep_flops(L, pb.M, 1, false, with_color), s, "FB_sweep");
  pick_bf_tile(bf_ti(L, RNB_VARIANT_BWD_TI_SHIFT), pb, [&](auto ti_c, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(bf_fb_kernel<decltype(ti_c)::value>, grid, block, 0, s, g);
  });
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

}  // namespace rnb
