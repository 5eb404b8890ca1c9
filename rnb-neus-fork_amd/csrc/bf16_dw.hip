// RNB_VARIANT_BF16: the weight gradients of one backward — every hidden-layer job of both networks in ONE grouped
// launch (bf_dw_kernel, + the ordered slab reduction of the deterministic variant), the plan that lists, splits and
// sizes it, and the gradient of the sdf-head row.  See bf16_common.hip.h.
#include "bf16_common.hip.h"

namespace rnb {

// ---------------------------------------------------------------------------------------------------------------
// dW: every weight-gradient job of one backward in one launch
// ---------------------------------------------------------------------------------------------------------------
// One job = dW[N x K] (+)= sum over pairs X_p^T Y_p, X_p [M x 256] K8 (all N = 256 columns), Y_p [M x Cy] K8 of which
// columns ycol0 .. ycol0 + K are used (K = 64 or 256).  A workgroup = 8 waves owns ALL of dW for one point range, so
// every operand byte is read once per launch: wave (wm, wn) computes rows 64 wm .. +64, columns (K / 2) wn .. of dW.
// Both MFMA operands are one 16-byte K8 unit per lane straight from global memory (see the header of this file).
struct BfDwJob {
  const bfraw* X[2];
  const bfraw* Y[2];
  int Cy[2], ycol0[2];
  int npairs, K, lddw, bias_pair;
  float* dW;        // fp32 [256 x lddw]
  float* db;        // fp32 [256] or nullptr
  float* part;      // deterministic: [splits][256][lddw] slabs (or nullptr: fp32 atomics)
  float* partb;     // deterministic: [splits][256]
};
struct BfDwGroup {
  BfDwJob job[kMaxBfDwJobs];
  int njobs, splits;
  int64_t M, rows_per_split;
};

// ---- the pieces the two job bodies share.  Lane (i, h) = (lane & 31, lane >> 5), wave (wm, wn) = (wave >> 1, wave & 1);
// accumulator (ti, tj, r) is dW[64 wm + 32 ti + (r & 3) + 8 (r >> 2) + 4 h][32 TN wn + 32 tj + i], bs[ti] the lane's part
// of db[64 wm + 32 ti + i].
// The K = 256 body sits at 240 VGPRs: how these pieces are cut decides whether bf_dw_kernel spills (the same step helper
// next to a hand-written zeroing loop spilt 84 VGPRs).  Check any change here with tools/codegen_compare.py. ----
template <int TN>
__device__ inline void bf_dw_zero(v16f (&acc)[2][TN]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// ragged tail: points >= M contribute nothing (their saved state is padding).  `a` holds points m0 + 8 h .. + 7 of a 16-point step.
__device__ inline void bf_dw_mask_tail(vu4 (&a)[2], int64_t m0, int64_t M, int h) {
  if (m0 + 16 > M) {
    const int64_t first = m0 + 8 * h;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      unsigned w[4] = {a[ti].x, a[ti].y, a[ti].z, a[ti].w};
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (first + j >= M) w[j >> 1] &= (j & 1) ? 0x0000ffffu : 0xffff0000u;
      a[ti] = vu4{w[0], w[1], w[2], w[3]};
    }
  }
}

// one 16-point step: tail mask, acc += a^T b on the matrix cores, bs += the column sums of a (the bias pair's X operand)
template <int TN>
__device__ inline void bf_dw_step(vu4 (&a)[2], const vu4 (&b)[TN], int64_t m0, int64_t M, int h, bool do_bias,
                                  v16f (&acc)[2][TN], float (&bs)[2]) {
  bf_dw_mask_tail(a, m0, M, h);
#pragma unroll
  for (int tj = 0; tj < TN; ++tj)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
      acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, a[ti]), __builtin_bit_cast(bf8, b[tj]),
                                                            acc[ti][tj], 0, 0, 0);
  if (do_bias) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const vu4 v = a[ti];
      bs[ti] += (bf_lo(v.x) + bf_hi(v.x)) + (bf_lo(v.y) + bf_hi(v.y)) + (bf_lo(v.z) + bf_hi(v.z)) + (bf_lo(v.w) + bf_hi(v.w));
    }
  }
}

// the job's sums of this point range leave: into slab `split` with plain stores (deterministic) or through fp32 atomics
template <int TN>
__device__ inline void bf_dw_store(const BfDwJob& J, int split, int wm, int wn, int i, int h, bool bias_wave,
                                   const v16f (&acc)[2][TN], const float (&bs)[2]) {
  const int lddw = J.lddw;
  float* __restrict__ pdst = J.part ? J.part + (size_t)split * FH * lddw : nullptr;
#pragma unroll
  for (int tj = 0; tj < TN; ++tj) {
    const int col = wn * (32 * TN) + tj * 32 + i;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (pdst) pdst[(size_t)row * lddw + col] = acc[ti][tj][r];
        else atomicAdd(J.dW + (size_t)row * lddw + col, acc[ti][tj][r]);
      }
  }
  if (bias_wave) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const float t = bs[ti] + __shfl_xor(bs[ti], 32, 64);
      if (h == 0) {
        const int row = wm * 64 + ti * 32 + i;
        if (J.partb) J.partb[(size_t)split * FH + row] = t;
        else atomicAdd(J.db + row, t);
      }
    }
  }
}

template <int KW>   // columns of dW per wave: 128 (K = 256) or 32 (K = 64)
__device__ inline void bf_dw_job(const BfDwJob& J, int64_t m_begin, int64_t m_end, int64_t M, int split, int lane, int wave) {
  constexpr int TN = KW / 32;
  const int wm = wave >> 1, wn = wave & 1;
  const int i = lane & 31, h = lane >> 5;
  v16f acc[2][TN];
  bf_dw_zero<TN>(acc);
  float bs[2] = {0.f, 0.f};
  const bool bias_wave = J.db != nullptr && wn == 0;
  for (int pi = 0; pi < J.npairs; ++pi) {
    const bfraw* Xb = J.X[pi] + ((size_t)(m_begin >> 3) * FH + wm * 64 + i) * 8;
    const bfraw* Yb = J.Y[pi] + ((size_t)(m_begin >> 3) * J.Cy[pi] + J.ycol0[pi] + wn * KW + i) * 8;
    const size_t xs = (size_t)FH * 8, ys = (size_t)J.Cy[pi] * 8;   // elements per 8-point block
    const bool do_bias = bias_wave && pi == J.bias_pair;
    const int64_t nsteps = (m_end - m_begin + 15) / 16;
    // 3-slot register ring: the loads of step s + 2 are issued before the MFMAs of step s (HBM latency x bandwidth per
    // CU is ~40 KB; one step of one workgroup is 16 KB of operands, two workgroup-steps are in flight per CU)
    vu4 a[3][2], b[3][TN];
    auto load = [&](int slot, int64_t s) {
      const int64_t sc = s < nsteps ? s : nsteps - 1;   // past the end: a harmless re-load of the last step
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) a[slot][ti] = *reinterpret_cast<const vu4*>(Xb + (2 * sc + h) * xs + ti * 32 * 8);
#pragma unroll
      for (int tj = 0; tj < TN; ++tj) b[slot][tj] = *reinterpret_cast<const vu4*>(Yb + (2 * sc + h) * ys + tj * 32 * 8);
    };
    auto compute = [&](int slot, int64_t s) { bf_dw_step<TN>(a[slot], b[slot], m_begin + s * 16, M, h, do_bias, acc, bs); };
    load(0, 0);
    load(1, 1);
    for (int64_t s = 0; s < nsteps; s += 3) {
      load(2, s + 2);
      compute(0, s);
      if (s + 1 < nsteps) { load(0, s + 3); compute(1, s + 1); }
      if (s + 2 < nsteps) { load(1, s + 4); compute(2, s + 2); }
    }
  }
  bf_dw_store<TN>(J, split, wm, wn, i, h, bias_wave, acc, bs);
}

// K = 256 jobs: the two operand chunks of 32 points (X 16 KB + Y 16 KB, K8 units in global order) are staged in LDS by
// LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, no VGPR round trip), three chunks deep, so every operand byte is
// fetched ONCE per workgroup (the register-direct form above lets the two / four waves that share a fragment each
// fetch it: measured 1.7x the unique bytes at the memory side).  One raw barrier per chunk; the DMAs of the next two
// chunks stay in flight across it (counted vmcnt, never 0 inside the loop).
constexpr int kDwChunk = 32;                            // points per chunk
constexpr int kDwOpBytes = (kDwChunk / 8) * FH * 16;    // bytes of one operand chunk (4 blocks x 256 units x 16 B)
constexpr int kDwBufs = 3;

__device__ inline void dw_issue_chunk(const bfraw* __restrict__ Xg, const bfraw* __restrict__ Yg, int64_t chunk,
                                      int64_t nchunks, int CyUnits, char* lds_buf, int wave, int lane) {
  // this wave's share: units [wave * 128, wave * 128 + 128) of each operand chunk = 2 DMA instructions per operand.
  // X chunk: blocks 4 chunk .. +3, all 256 columns: contiguous in global.  Y chunk: 256 of the Cy columns per block.
  const int64_t c = chunk < nchunks ? chunk : nchunks - 1;   // past the end: harmless re-fetch, keeps vmcnt uniform
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int u = wave * 128 + q * 64;     // first unit of this instruction (wave-uniform); blk = u / 256, col = u % 256
    const int blk = u >> 8, col = (u & 255) + lane;
    const bfraw* xs = Xg + ((size_t)(c * 4 + blk) * FH + col) * 8;
    const bfraw* ys = Yg + ((size_t)(c * 4 + blk) * CyUnits + col) * 8;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)xs,
                                     (__attribute__((address_space(3))) void*)(lds_buf + u * 16), 16, 0, RNB_AUX_LD);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ys,
                                     (__attribute__((address_space(3))) void*)(lds_buf + kDwOpBytes + u * 16), 16, 0, RNB_AUX_LD);
  }
}

__device__ inline void bf_dw_job_lds(const BfDwJob& J, int64_t m_begin, int64_t m_end, int64_t M, int split, int lane, int wave,
                                     char* lds) {
  constexpr int TN = 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int i = lane & 31, h = lane >> 5;
  v16f acc[2][TN];
  bf_dw_zero<TN>(acc);
  float bs[2] = {0.f, 0.f};
  const bool bias_wave = J.db != nullptr && wn == 0;
  const int64_t nchunks = (m_end - m_begin + kDwChunk - 1) / kDwChunk;   // (ranges are multiples of 64 points)
  for (int pi = 0; pi < J.npairs; ++pi) {
    const bfraw* Xg = J.X[pi] + (size_t)(m_begin >> 3) * FH * 8;
    const bfraw* Yg = J.Y[pi] + ((size_t)(m_begin >> 3) * J.Cy[pi] + J.ycol0[pi]) * 8;
    const bool do_bias = bias_wave && pi == J.bias_pair;
    __builtin_amdgcn_s_barrier();   // every wave is done with the buffers of the previous pair
    dw_issue_chunk(Xg, Yg, 0, nchunks, J.Cy[pi], lds, wave, lane);
    dw_issue_chunk(Xg, Yg, 1, nchunks, J.Cy[pi], lds + 2 * kDwOpBytes, wave, lane);
    for (int64_t c = 0; c < nchunks; ++c) {
      // chunk c has landed (this wave's 4 DMAs of chunk c + 1 may still be in flight) ...
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __builtin_amdgcn_s_barrier();   // ... for every wave; and every wave has finished reading chunk c - 1
      dw_issue_chunk(Xg, Yg, c + 2, nchunks, J.Cy[pi], lds + ((c + 2) % kDwBufs) * 2 * kDwOpBytes, wave, lane);
      const char* bx = lds + (c % kDwBufs) * 2 * kDwOpBytes;
      const char* by = bx + kDwOpBytes;
#pragma unroll
      for (int st = 0; st < 2; ++st) {   // two 16-point MFMA steps per chunk
        vu4 a[2], b[TN];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
          a[ti] = *reinterpret_cast<const vu4*>(bx + ((2 * st + h) * FH + wm * 64 + ti * 32 + i) * 16);
#pragma unroll
        for (int tj = 0; tj < TN; ++tj)
          b[tj] = *reinterpret_cast<const vu4*>(by + ((2 * st + h) * FH + wn * 128 + tj * 32 + i) * 16);
        bf_dw_step<TN>(a, b, m_begin + c * kDwChunk + st * 16, M, h, do_bias, acc, bs);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's LDS reads of chunk c are complete
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the two over-fetched chunks before the buffers are reused
  }
  bf_dw_store<TN>(J, split, wm, wn, i, h, bias_wave, acc, bs);
}

__global__ __launch_bounds__(512, 1) void bf_dw_kernel(const BfDwGroup g) {
  __shared__ __attribute__((aligned(16))) char lds[kDwBufs * 2 * kDwOpBytes];   // 96 KB: the ONLY shared object
  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  const int ji = blockIdx.x / g.splits, split = blockIdx.x - ji * g.splits;
  const BfDwJob& J = g.job[ji];
  const int64_t m_begin = (int64_t)split * g.rows_per_split;
  const int64_t m_end = m_begin + g.rows_per_split < g.M ? m_begin + g.rows_per_split : g.M;
  if (m_begin >= m_end) return;
  if (J.K == 256) bf_dw_job_lds(J, m_begin, m_end, g.M, split, lane, wave, lds);
  else bf_dw_job<32>(J, m_begin, m_end, g.M, split, lane, wave);
}

// deterministic variant: ordered reduction of the slabs
__global__ __launch_bounds__(256) void bf_dw_reduce_kernel(const BfDwGroup g) {
  const BfDwJob& J = g.job[blockIdx.y];
  const size_t n = (size_t)FH * J.lddw;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (size_t)gridDim.x * 256) {
    if ((int)(idx % J.lddw) >= J.K) continue;
    double s = 0.0;
    for (int sp = 0; sp < g.splits; ++sp) s += (double)J.part[(size_t)sp * n + idx];
    J.dW[idx] = (float)s;
  }
  if (J.db != nullptr && J.partb != nullptr) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < FH; r += gridDim.x * 256) {
      double s = 0.0;
      for (int sp = 0; sp < g.splits; ++sp) s += (double)J.partb[(size_t)sp * FH + r];
      J.db[r] = (float)s;
    }
  }
}

// gradient of the sdf-head row: dw_sdf[k] += sum_rows (sbar / scale * a_last + u_last), db_sdf += sum sbar / scale.
// One thread per column and point slab; K8 units (8 points of one column) per load.  One slab per column chunk in the
// deterministic variant (a single add onto zero per address).
__global__ __launch_bounds__(1024) void bf_sdf_head_bwd_kernel(const bfraw* __restrict__ a, const bfraw* __restrict__ ulast,
                                                               const float* __restrict__ sbar, float inv_scale, int64_t M,
                                                               int64_t rows_per_blk, float* __restrict__ dwsdf,
                                                               float* __restrict__ dbsdf) {
  __shared__ double red[4][FH], redb[4];
  const int c = threadIdx.x & 255, ph = threadIdx.x >> 8;   // column, one of 4 row phases (8-point blocks ph, ph + 4, ...)
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk;
  const int64_t r1 = r0 + rows_per_blk < M ? r0 + rows_per_blk : M;
  double s = 0.0, sb = 0.0;
  for (int64_t r = r0 + 8 * ph; r < r1; r += 32) {
    const vu4 av = *reinterpret_cast<const vu4*>(a + ((size_t)(r >> 3) * FH + c) * 8);
    const vu4 uv = *reinterpret_cast<const vu4*>(ulast + ((size_t)(r >> 3) * FH + c) * 8);
    const float af[8] = {bf_lo(av.x), bf_hi(av.x), bf_lo(av.y), bf_hi(av.y), bf_lo(av.z), bf_hi(av.z), bf_lo(av.w), bf_hi(av.w)};
    const float uf[8] = {bf_lo(uv.x), bf_hi(uv.x), bf_lo(uv.y), bf_hi(uv.y), bf_lo(uv.z), bf_hi(uv.z), bf_lo(uv.w), bf_hi(uv.w)};
    float t = 0.f, tb = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (r + j < r1) {
        const float w = sbar[r + j] * inv_scale;
        t += fmaf(w, af[j], uf[j]);
        tb += w;
      }
    }
    s += (double)t;
    sb += (double)tb;
  }
  red[ph][c] = s;
  if (c == 0) redb[ph] = sb;
  __syncthreads();
  if (ph == 0) {
    atomicAdd(dwsdf + c, (float)(red[0][c] + red[1][c] + red[2][c] + red[3][c]));
    if (c == 0) atomicAdd(dbsdf, (float)(redb[0] + redb[1] + redb[2] + redb[3]));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// gradient of the sdf-head row (reads a_last, u_nh of the RA sweep and pb.sbar)
int bf16_sdf_head_bwd(const Layout& L, PointBufs& pb, float* packed_grad, hipStream_t s) {
  const int64_t M = pb.M, rows_per_blk = bf_rows_per_slab(L, M);
  hipLaunchKernelGGL(bf_sdf_head_bwd_kernel, dim3((unsigned)((M + rows_per_blk - 1) / rows_per_blk)), dim3(1024), 0, s,
                     reinterpret_cast<const bfraw*>(pb.a[L.nh - 1]), reinterpret_cast<const bfraw*>(pb.u[L.nh]), pb.sbar,
                     1.f / L.sdf_scale, M, rows_per_blk, packed_grad + L.wsdf_off, packed_grad + L.bsdf_off);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// The weight-gradient jobs of one bf16 backward, in the launch order of bf16_dw_shapes (bf16_dw_plan.h: which jobs, their
// column ranges and pitches): here each gets its operands and targets.  f(job, flops) gets every field but the slabs.
// Sizing lists a PointBufs without buffers and no packed gradient: the operands and targets are then null.
// (Not dw.hip's dw_list: other operands, formats, kernels and order.)
template <class F>
static void bf16_dw_list(const Layout& L, const PointBufs& pb, const BfDwShape* shape, int nshapes, float* packed_grad, F f) {
  const int64_t M = pb.M;
  auto bf = [](const void* p) { return reinterpret_cast<const bfraw*>(p); };
  for (int q = 0; q < nshapes; ++q) {
    const BfDwShape& sh = shape[q];
    const int l = sh.layer;
    const void *X1 = nullptr, *Y1 = nullptr, *X2 = nullptr, *Y2 = nullptr;
    int Cy = FH;
    const Lin* ln = nullptr;
    double fl = 0.0;
    switch (sh.kind) {
      case BF_DW_HIDDEN:   // pairs gz_l / u_l and zb_l / in_l
        ln = &L.hid[l];
        Cy = l == 0 ? L.Ep : FH;
        X1 = pb.gz[l]; Y1 = l == 0 ? (const void*)pb.u0_k8 : (const void*)pb.u[l];
        X2 = pb.zb[l]; Y2 = l == 0 ? (const void*)pb.e : (const void*)pb.a[l - 1];
        fl = 4.0 * (double)M * ln->N * ln->K;
        break;
      case BF_DW_FEAT:
        ln = &L.feat;
        X1 = pb.fbar_k8; Y1 = pb.a[L.nh - 1];
        fl = 2.0 * (double)M * ln->N * ln->K;
        break;
      case BF_DW_ALBEDO_HIDDEN:   // dW_l = zc_l^T in_l
        ln = &L.col[l];
        X1 = pb.zc8[l]; Y1 = pb.ac8[l - 1];
        fl = 2.0 * (double)M * ln->N * ln->K;
        break;
      default:   // the albedo net's layer 0 on the Cinp-wide input: BF_DW_ALBEDO_IN_FEAT (its flops count the whole layer), _PE
        ln = &L.col[0];
        Cy = L.Cinp;
        X1 = pb.zc8[0]; Y1 = pb.cin8;
        fl = sh.kind == BF_DW_ALBEDO_IN_FEAT ? 2.0 * (double)M * ln->N * ln->K : 0.0;
        break;
    }
    BfDwJob J;
    memset(&J, 0, sizeof(J));
    J.X[0] = bf(X1); J.Y[0] = bf(Y1); J.Cy[0] = Cy; J.ycol0[0] = sh.ycol0;
    J.X[1] = bf(X2); J.Y[1] = bf(Y2); J.Cy[1] = sh.npairs == 2 ? Cy : 0; J.ycol0[1] = sh.ycol0;
    J.npairs = sh.npairs; J.K = sh.K; J.lddw = sh.lddw; J.bias_pair = sh.bias_pair;
    if (packed_grad != nullptr) {
      J.dW = packed_grad + ln->w_off + sh.ycol0;      // a column range [ycol0, ycol0 + K) of the layer's [256 x Kp] gradient
      J.db = sh.with_bias ? packed_grad + ln->b_off : nullptr;
    }
    f(J, fl);
  }
}

// The one plan of the grouped launch: what is launched, how the points are split and where each job's slabs lie.
struct BfDwPlan {
  BfDwGroup grp;                       // the jobs in launch order (slab pointers unset), splits, rows_per_split
  int njobs;                           // jobs listed (grp.njobs holds at most kMaxBfDwJobs of them)
  int64_t slab_off[kMaxBfDwJobs];      // deterministic: float offset of the job's [splits][256][lddw] slabs in pb.dw_part;
                                       // its [splits][256] bias slabs follow them
  int64_t total;                       // floats of all slabs
  double flops;
};
static BfDwPlan bf16_dw_plan(const Layout& L, const PointBufs& pb, bool with_color, float* packed_grad) {
  BfDwPlan P;
  memset(&P, 0, sizeof(P));
  P.grp.M = pb.M;
  BfDwShape shape[kBfDwListed];
  P.njobs = bf16_dw_shapes(bf16_dw_net(L), with_color, shape);
  bf16_dw_list(L, pb, shape, P.njobs, packed_grad, [&](const BfDwJob& J, double fl) {
    if (P.grp.njobs < kMaxBfDwJobs) P.grp.job[P.grp.njobs++] = J;
    P.flops += fl;
  });
  const BfDwSplit S = bf16_dw_split(shape, P.njobs, pb.M);
  P.grp.rows_per_split = S.rows_per_split;
  P.grp.splits = S.splits;
  P.total = S.total;
  for (int q = 0; q < kMaxBfDwJobs; ++q) P.slab_off[q] = S.slab_off[q];
  return P;
}

// floats of bf16_dw_backward's ordered-reduction slabs over M points (deterministic variant)
int64_t bf16_dw_floats(const Layout& L, int64_t M, bool with_color) {
  PointBufs pb{};
  pb.M = M;
  return bf16_dw_plan(L, pb, with_color, nullptr).total;
}

// every dW job of the SDF network (+ the feature head's, + the bf16 albedo net's hidden layers) of one backward
int bf16_dw_backward(const Layout& L, PointBufs& pb, bool with_color, float* packed_grad, hipStream_t s) {
  BfDwPlan P = bf16_dw_plan(L, pb, with_color, packed_grad);
  BfDwGroup& grp = P.grp;
  if (P.njobs > kMaxBfDwJobs) RNB_FAIL(RNB_E_INVALID, "too many weight-gradient jobs for one bf16 launch");
  const bool det = (L.variant & RNB_VARIANT_DETERMINISTIC) != 0;
  // (the staged fp32 kernel's slabs at the tail of the workspace are free again: its reduction was enqueued earlier)
  if (det) {
    if (P.total > pb.dw_part_floats) RNB_FAIL(RNB_E_WORKSPACE, "deterministic bf16 dW: partial-slab workspace exhausted");
    RNB_CHECK_HIP(hipMemsetAsync(pb.dw_part, 0, (size_t)pb.dw_part_floats * sizeof(float), s));
    for (int q = 0; q < grp.njobs; ++q) {
      grp.job[q].part = pb.dw_part + P.slab_off[q];
      grp.job[q].partb = grp.job[q].part + (int64_t)grp.splits * FH * grp.job[q].lddw;
    }
  }
  ProfScope prof(P.flops, s, "dW(all)");
  hipLaunchKernelGGL(bf_dw_kernel, dim3((unsigned)(grp.njobs * grp.splits)), dim3(512), 0, s, grp);
  RNB_CHECK_LAUNCH();
  if (det) {
    hipLaunchKernelGGL(bf_dw_reduce_kernel, dim3(64, grp.njobs), dim3(256), 0, s, grp);
    RNB_CHECK_LAUNCH();
  }
  return RNB_OK;
}

}  // namespace rnb
