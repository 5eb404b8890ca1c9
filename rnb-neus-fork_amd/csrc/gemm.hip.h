// fp32 MFMA GEMM building blocks for gfx950 (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fma chain).
//
// One workgroup = 256 threads = 4 wave64 arranged 2(M) x 2(N); block tile 128 x BN (BN = 128 or 256),
// K-step 32; each wave owns a 64 x BN/2 sub-tile = 2 x TN MFMA tiles of 32x32 (16 accumulator registers
// per tile per lane).  Operand tiles are staged through LDS with a register prefetch of the next K-step
// (global loads in flight while the matrix cores run).  fp32 MFMA retires 2 k per 64 cycles per SIMD, so
// operand bandwidth is far from binding; the layouts are chosen for conflict-free ds_read_b128 /
// ds_read_b32.  All tile/wave indices are kept in SGPRs (readfirstlane) so every MFMA runs with full
// EXEC and no per-instruction branching; partially filled column blocks take a separate guarded path.
//
// The reduction index inside a K-step is permuted: within each group of 8 k, lane half h (= lane>>5)
// supplies k = 8q+4h+c for MFMA step c (one 16-byte LDS read feeds 4 MFMAs).  A and B use the same
// permutation, so the product is unchanged up to fp32 summation order.
#pragma once
#include <hip/hip_runtime.h>

#include "dw_plan.h"

namespace rnb {

typedef float v16f __attribute__((ext_vector_type(16)));
// native 4-vector for register staging (HIP's float4 struct is not split by SROA when it sits in an
// array: the staging arrays then live in scratch memory)
typedef float vf4 __attribute__((ext_vector_type(4)));
__device__ inline vf4 make_vf4(float a, float b, float c, float d) {
  vf4 r = {a, b, c, d};
  return r;
}

constexpr int BM = 128;   // (BK, the points per main-loop step: dw_plan.h)
constexpr int LDK = BK + 4;   // pitch (floats) of a k-contiguous tile  [rows][36]

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter,
// i.e. it would wait for prefetch loads and fire-and-forget global stores that are still in flight.
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ inline int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Raw buffer access to one tile of a row-major matrix: resource = tile base + byte size, per-lane 32-bit
// byte offset in a VGPR, wave-uniform byte offset in the scalar operand (no per-access vector address
// arithmetic; out-of-range reads return 0, out-of-range writes are dropped).
#ifndef RNB_AUX_ST
#define RNB_AUX_ST 2   // nt: the saved state is written once and read much later (or once): keep it out of L2's way
#endif
#ifndef RNB_AUX_LD
#define RNB_AUX_LD 2   // nt: epilogue operand tiles are read exactly once
#endif
typedef __amdgpu_buffer_rsrc_t BufRsrc;
typedef float vf2 __attribute__((ext_vector_type(2)));
typedef unsigned vu2 __attribute__((ext_vector_type(2)));
__device__ inline BufRsrc tile_rsrc(const float* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, p ? bytes : 0, 0x00020000);
}
__device__ inline void bstore(BufRsrc r, unsigned voff, unsigned soff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, RNB_AUX_ST);
}
__device__ inline float bload(BufRsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, RNB_AUX_LD));
}
__device__ inline vf2 bload2(BufRsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(vf2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}

// ---- global -> register staging ------------------------------------------------------------------
// k-contiguous source: element (r, k) at src[r*ld + k]; tile = ROWS rows from r0, k0..k0+31.
template <int ROWS, bool GUARD>
__device__ inline void load_rows(const float* __restrict__ src, int ld, int r0, int k0, int rmax, int tid,
                                 vf4 (&v)[ROWS / 32]) {
#pragma unroll
  for (int i = 0; i < ROWS / 32; ++i) {
    const int idx = tid + 256 * i;
    const int r = idx >> 3, c4 = idx & 7;
    if constexpr (!GUARD) {
      v[i] = *reinterpret_cast<const vf4*>(src + (size_t)(r0 + r) * ld + k0 + c4 * 4);
    } else {   // branch-free: load from a clamped (valid) row, then select
      const bool ok = r0 + r < rmax;
      const int rr = ok ? r0 + r : rmax - 1;
      const vf4 t = *reinterpret_cast<const vf4*>(src + (size_t)rr * ld + k0 + c4 * 4);
      v[i] = make_vf4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
    }
  }
}
template <int ROWS>
__device__ inline void store_rows(float* __restrict__ T, int tid, const vf4 (&v)[ROWS / 32]) {
#pragma unroll
  for (int i = 0; i < ROWS / 32; ++i) {
    const int idx = tid + 256 * i;
    const int r = idx >> 3, c4 = idx & 7;
    *reinterpret_cast<vf4*>(T + r * LDK + c4 * 4) = v[i];
  }
}
// k-major source: element (k, c) at src[k*ld + c]; tile = 32 k rows from k0, COLS columns from c0.
template <int COLS, bool GUARD>
__device__ inline void load_kmajor(const float* __restrict__ src, int ld, int k0, int c0, int kmax, int cmax,
                                   int tid, vf4 (&v)[COLS / 32]) {
  constexpr int C4 = COLS / 4;   // vf4 per k row
#pragma unroll
  for (int i = 0; i < COLS / 32; ++i) {
    const int idx = tid + 256 * i;
    const int kk = idx / C4, c4 = idx % C4;
    if constexpr (!GUARD) {
      v[i] = *reinterpret_cast<const vf4*>(src + (size_t)(k0 + kk) * ld + c0 + c4 * 4);
    } else {   // branch-free: clamp to a valid element, then select
      const bool ok = (k0 + kk < kmax) && (c0 + c4 * 4 < cmax);
      const int kr = k0 + kk < kmax ? k0 + kk : kmax - 1;
      const int cc = c0 + c4 * 4 < cmax ? c0 + c4 * 4 : cmax - 4;
      const vf4 t = *reinterpret_cast<const vf4*>(src + (size_t)kr * ld + cc);
      v[i] = make_vf4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
    }
  }
}
template <int COLS>
__device__ inline void store_kmajor(float* __restrict__ T, int tid, const vf4 (&v)[COLS / 32]) {
  constexpr int C4 = COLS / 4;
#pragma unroll
  for (int i = 0; i < COLS / 32; ++i) {
    const int idx = tid + 256 * i;
    const int kk = idx / C4, c4 = idx % C4;
    *reinterpret_cast<vf4*>(T + kk * COLS + c4 * 4) = v[i];
  }
}

// ---- LDS -> MFMA fragments ---------------------------------------------------------------------
// PITCH: LDK for k-contiguous tiles, the tile width for k-major tiles.
template <bool KMAJOR, int PITCH>
__device__ inline void frag4(const float* __restrict__ T, int idx, int q, int h, float (&o)[4]) {
  if constexpr (!KMAJOR) {
    const vf4 t = *reinterpret_cast<const vf4*>(T + idx * PITCH + q * 8 + h * 4);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = T[(q * 8 + h * 4 + c) * PITCH + idx];
  }
}

// One K-step (32 k) of a wave's 64 x (32*TN) sub-tile.  `mask` bit j = column tile j is inside N
// (wave-uniform, only consulted when GUARD).
template <bool A_KMAJOR, int A_PITCH, bool B_KMAJOR, int B_PITCH, int TN, bool GUARD>
__device__ inline void mma_step(const float* __restrict__ As, const float* __restrict__ Bs, int a_base, int b_base,
                                int lane, unsigned mask, v16f (&acc)[2][TN]) {
  const int i = lane & 31, h = lane >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float a[2][4], b[TN][4];
    frag4<A_KMAJOR, A_PITCH>(As, a_base + i, q, h, a[0]);
    frag4<A_KMAJOR, A_PITCH>(As, a_base + 32 + i, q, h, a[1]);
#pragma unroll
    for (int tj = 0; tj < TN; ++tj) frag4<B_KMAJOR, B_PITCH>(Bs, b_base + 32 * tj + i, q, h, b[tj]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int tj = 0; tj < TN; ++tj) {
        if (!GUARD || ((mask >> tj) & 1u)) {
          acc[0][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0][c], b[tj][c], acc[0][tj], 0, 0, 0);
          acc[1][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1][c], b[tj][c], acc[1][tj], 0, 0, 0);
        }
      }
    }
    // keep the fragment loads of the next k-group behind this group's MFMAs: hoisting all four groups'
    // ds_reads to the top costs 4x the fragment registers and spills the staging registers
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Accumulator element (tile ti ; register r) of lane `lane` -> row inside the wave's 64-row band.
__device__ inline int acc_row(int ti, int r, int lane) { return ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Epilogue through LDS: the MFMA accumulator layout (one column per lane, rows spread over registers)
// would make every global access a 4-byte-per-lane access of two 128-byte row segments.  Each wave
// instead transposes its sub-tile through a private LDS strip, 16 rows at a time, and then walks it
// row-major with 16 bytes per lane: the epilogue functor sees 4 consecutive columns of one row
// (`epi.apply4(row, col, v)`, col % 4 == 0) and issues dwordx4 loads/stores (512 contiguous bytes per
// half-wave).  `strip` = this wave's [16][32*TN + 4] floats of the (now idle) staging LDS.
template <int TN, class Epi, int TI = 2>
__device__ inline void run_epilogue(const v16f (&acc)[TI][TN], float* __restrict__ strip, int row0, int col0,
                                    int lane, unsigned mask, const Epi& epi) {
  constexpr int W = 32 * TN;   // columns of the wave's sub-tile
  constexpr int P = W + 4;     // strip pitch (floats)
  constexpr int C4 = W / 4;    // 16-byte groups per row
  const int h = lane >> 5, cl = lane & 31;
#pragma unroll
  for (int ti = 0; ti < TI; ++ti) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      // registers 8*half .. 8*half+7 of every column tile hold rows 16*half .. 16*half+15
#pragma unroll
      for (int tj = 0; tj < TN; ++tj) {
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
          const int rl = (rr & 3) + 8 * (rr >> 2) + 4 * h;
          strip[rl * P + tj * 32 + cl] = acc[ti][tj][half * 8 + rr];
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int it = 0; it < W / 16; ++it) {
        const int idx = it * 64 + lane;
        const int rl = idx / C4, c4 = idx % C4;
        const vf4 v = *reinterpret_cast<const vf4*>(strip + rl * P + c4 * 4);
        if ((mask >> (c4 >> 3)) & 1u) epi.apply4(row0 + ti * 32 + half * 16 + rl, col0 + c4 * 4, v);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <int TN>
__device__ inline void zero_acc(v16f (&acc)[2][TN]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// ---- C[M x N] = A[M x K] * op(B) ------------------------------------------------------------------
//   B_KMAJOR == false ("NT"): B given as W[N][K] (k contiguous): C = A W^T      (forward-shaped layers)
//   B_KMAJOR == true  ("NN"): B given as W[K][N] (n contiguous): C = A W        (reverse-shaped layers)
// M is a multiple of 128 (padded buffers), N and K multiples of 32.  grid = (M/128, ceil(N/BN)).
template <bool B_KMAJOR, int BN, bool GUARD>
__device__ inline void rows_main_loop(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw,
                                      int N, int K, int m_blk, int n_blk, int wm, int wn, unsigned mask,
                                      float* __restrict__ As, float* __restrict__ Bs, v16f (&acc)[2][BN / 64]) {
  constexpr int TN = BN / 64;
  constexpr int B_PITCH = B_KMAJOR ? BN : LDK;
  const int tid = threadIdx.x, lane = tid & 63;
  vf4 ra[BM / 32], rb[BN / 32];
  const int nk = K / BK;
  if (nk > 0) {
    load_rows<BM, false>(A, lda, m_blk, 0, 0, tid, ra);
    if constexpr (!B_KMAJOR) load_rows<BN, GUARD>(W, ldw, n_blk, 0, N, tid, rb);
    else load_kmajor<BN, GUARD>(W, ldw, 0, n_blk, K, N, tid, rb);
  }
  for (int kt = 0; kt < nk; ++kt) {
    store_rows<BM>(As, tid, ra);
    if constexpr (!B_KMAJOR) store_rows<BN>(Bs, tid, rb);
    else store_kmajor<BN>(Bs, tid, rb);
    lds_barrier();
    if (kt + 1 < nk) {
      const int k0 = (kt + 1) * BK;
      load_rows<BM, false>(A, lda, m_blk, k0, 0, tid, ra);
      if constexpr (!B_KMAJOR) load_rows<BN, GUARD>(W, ldw, n_blk, k0, N, tid, rb);
      else load_kmajor<BN, GUARD>(W, ldw, k0, n_blk, K, N, tid, rb);
    }
    mma_step<false, LDK, B_KMAJOR, B_PITCH, TN, GUARD>(As, Bs, wm * 64, wn * (BN / 2), lane, mask, acc);
    lds_barrier();
  }
}

// GUARD (chosen by the host: N % BN != 0) selects the variant whose B staging is bounds-checked and whose
// MFMAs are skipped for column tiles outside N.  One variant per kernel: two inlined copies of the main
// loop in one kernel exceed the backend's alloca-promotion budget and push the staging registers to scratch.
template <bool B_KMAJOR, int BN, bool GUARD, class Epi>
__global__ __launch_bounds__(256, BN == 256 ? 2 : 3) void gemm_rows_kernel(const float* __restrict__ A, int lda,
                                                                           const float* __restrict__ W, int ldw,
                                                                           int N, int K, Epi epi) {
  constexpr int TN = BN / 64;
  constexpr int B_FLOATS = B_KMAJOR ? BK * BN : BN * LDK;
  __shared__ __attribute__((aligned(16))) float smem[BM * LDK + B_FLOATS];
  float* As = smem;
  float* Bs = smem + BM * LDK;
  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  const int m_blk = blockIdx.x * BM, n_blk = blockIdx.y * BN;
  // column tiles of this wave that lie inside N (wave-uniform)
  unsigned mask = 0;
#pragma unroll
  for (int tj = 0; tj < TN; ++tj)
    if (n_blk + wn * (BN / 2) + tj * 32 < N) mask |= 1u << tj;

  v16f acc[2][TN];
  zero_acc<TN>(acc);
  rows_main_loop<B_KMAJOR, BN, GUARD>(A, lda, W, ldw, N, K, m_blk, n_blk, wm, wn, mask, As, Bs, acc);
  // the main loop ends with a barrier: the staging tiles are idle and become the transpose strips
  static_assert(4 * 16 * (32 * TN + 4) <= BM * LDK + B_FLOATS, "epilogue strips must fit in the staging LDS");
  run_epilogue<TN, Epi>(acc, smem + wave * 16 * (32 * TN + 4), m_blk + wm * 64, n_blk + wn * (BN / 2), lane, mask,
                        epi);
}

// ---- fp32 products as bf16 MFMA terms ("x3"): primitives (the scheme is described in fused_common.hip.h) ----------
typedef unsigned short x3raw;
typedef unsigned vu4x __attribute__((ext_vector_type(4)));
typedef __bf16 x3bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 x3bf2 __attribute__((ext_vector_type(2)));

__device__ inline unsigned x3_pack2(float a, float b) {
  x3bf2 p = {(__bf16)a, (__bf16)b};   // v_cvt_pk_bf16_f32, round to nearest even
  return __builtin_bit_cast(unsigned, p);
}
// 8 consecutive k of one row -> the row's hi / mid / lo operand registers: 3 conversions, 4 unpacks and 4 subtractions
// per pair.  The subtractions (exact) must stay scalar: beside MFMAs a v_pk_add_f32 costs ~13 cycles more than the two
// v_sub_f32 it replaces (MI355X_MICROARCH.md, packed f32 VALU), and hipcc's SLP pass would pack two adjacent
// subtractions — so one of each pair is written as an fma, which it cannot merge with the other.
__device__ inline void x3_split8(const vf4& x0, const vf4& x1, vu4x& hi, vu4x& mid, vu4x& lo) {
  const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float a = x[2 * p], b = x[2 * p + 1];
    unsigned uh = x3_pack2(a, b);
    asm("" : "+v"(uh));   // one conversion per pair (otherwise the low half is converted a second time for `uh << 16`)
    const float ra = a - __builtin_bit_cast(float, uh << 16);
    const float rb = __builtin_fmaf(__builtin_bit_cast(float, uh & 0xffff0000u), -1.f, b);
    unsigned um = x3_pack2(ra, rb);
    asm("" : "+v"(um));
    const float sa = ra - __builtin_bit_cast(float, um << 16);
    const float sb = __builtin_fmaf(__builtin_bit_cast(float, um & 0xffff0000u), -1.f, rb);
    hi[p] = uh;
    mid[p] = um;
    lo[p] = x3_pack2(sa, sb);
  }
}
// ---- maxima of adjoint tensors (scales of the x2h weight-gradient jobs) --------------------------------------------
// A producer of an adjoint tensor leaves max |.| over the REAL rows (padding rows hold workspace garbage) in a slot of
// PointBufs::amax as float bits (non-negative floats order like unsigned integers): one atomic per wave.
__device__ inline void amax_commit(unsigned* slot, float m, int lane) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  // fire and forget (the result is unused: the instruction does not return, the wave does not wait).  Callers keep the number
  // of atomics per slot and launch in the thousands: every wave of a 65,536-row GEMM sending one at the same moment (round 4's
  // first version) serialised in the L2 for 35 us.
  if (lane == 0 && slot != nullptr)
    (void)__hip_atomic_fetch_max(slot, __builtin_bit_cast(unsigned, m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// max |acc| over the accumulator rows below `rows_ok` (relative to the wave's first row) of a (32 TI) x (32 TJ) block
template <int TI, int TJ>
__device__ inline float acc_absmax(const v16f (&acc)[TI][TJ], int lane, int rows_ok) {
  float m0 = 0.f, m1 = 0.f;
  if (rows_ok >= 32 * TI) {
#pragma unroll
    for (int ti = 0; ti < TI; ++ti)
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          m0 = fmaxf(m0, fabsf(acc[ti][tj][r]));
          m1 = fmaxf(m1, fabsf(acc[ti][tj][r + 1]));
        }
  } else {
    const int h = lane >> 5;
#pragma unroll
    for (int ti = 0; ti < TI; ++ti)
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          m0 = fmaxf(m0, row < rows_ok ? fabsf(acc[ti][tj][r]) : 0.f);
        }
  }
  return fmaxf(m0, m1);
}

// ---- "x2h": the same idea on the fp16 matrix pipe with TWO planes and THREE terms ----------------------------------
// xs = x * S (S a power of two: exact), hi = fp16(xs), lo = fp16(xs - hi): two 11-bit roundings, |xs - hi - lo| <= 2^-22 |xs|
// (rms 2^-23.6: about four times the rounding noise of storing x in fp32 at all) as long as lo is a normal fp16 number
// (|xs| >= 2^-3), and <= 2^-25 absolutely below that; hi overflows at |xs| >= 65520.  a b is taken as
// a_hi b_hi + a_hi b_lo + a_lo b_hi (the dropped a_lo b_lo is below 2^-22 |a b|), at HALF the matrix time of the six bf16
// terms.  These per-product errors are independent and far below what the fp32 accumulation of a K = 256 dot product
// commits (2.7 ulp rms, profiles/r04_sdf_bias.txt): measured on the full network, the SDF comes out closer to fp64 than
// with the six bf16 terms (rms 8.3e-8 against 1.07e-7, profiles/r04_x2h_check.txt).  What bf16 gave for free — range — is
// bought with the scales, and every scale is taken from the data it scales (round 5; fused_common.hip.h, "per-tile scale"):
// per matrix for the weights (2^8 while max |w| < 64), per 64-point tile and layer for activations, network inputs and the
// reverse sweep's Jacobian rows (2^6 while the tile stays below 256), from recorded maxima for loss adjoints and for the saved
// state the weight-gradient kernel reads.  No operand has a range to respect.  (The RA sweep alone stays on the bf16 scheme.)
typedef _Float16 x2h8 __attribute__((ext_vector_type(8)));
typedef _Float16 x2h2 __attribute__((ext_vector_type(2)));
constexpr float kH2ActScale = 64.f, kH2WScale = 256.f;
__device__ inline unsigned x2h_pack2(float a, float b) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f2{a, b}, x2h2));   // v_cvt_pk_f16_f32, round to nearest even
}
// x - (float)(low / high half of h) in one instruction (v_fma_mix_f32 reads the fp16 half directly)
__device__ inline float x2h_resid_lo(float x, unsigned h) {
  float r;
  asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x), "v"(h));
  return r;
}
__device__ inline float x2h_resid_hi(float x, unsigned h) {
  float r;
  asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x), "v"(h));
  return r;
}
// the power-of-two scale of the adjoint operand of an x2h job: its maximum (float bits `mbits`) goes to [2^13, 2^14)
__device__ inline void x2h_dyn_scale(unsigned mbits, float& s, float& inv_s) {
  int ef = (int)(mbits >> 23);                        // biased exponent of the maximum (0: all zero)
  ef = ef < 24 ? 24 : (ef > 250 ? 250 : ef);          // both factors stay normal numbers
  s = __builtin_bit_cast(float, (unsigned)(267 - ef) << 23);        // 2^(13 - e)
  inv_s = __builtin_bit_cast(float, (unsigned)(ef - 13) << 23);     // 2^(e - 13)
}
// 8 consecutive k of one row (already scaled) -> hi / lo operand registers: 4 instructions per pair
__device__ inline void x2h_split8(const vf4& x0, const vf4& x1, vu4x& hi, vu4x& lo) {
  const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const unsigned uh = x2h_pack2(x[2 * p], x[2 * p + 1]);
    hi[p] = uh;
    lo[p] = x2h_pack2(x2h_resid_lo(x[2 * p], uh), x2h_resid_hi(x[2 * p + 1], uh));
  }
}
// planes -> operand registers of one row, either scheme
template <int NP>
__device__ inline void xn_split8(const vf4& x0, const vf4& x1, vu4x (&p)[NP]) {
  if constexpr (NP == 3) x3_split8(x0, x1, p[0], p[1], p[2]);
  else x2h_split8(x0, x1, p[0], p[1]);
}
// the six (three) terms of one 16-k step, small ones first, the (ti, tj) accumulators in rotation
template <int TI, int TJ, bool FIRST, int NP = 3>
__device__ inline void x3_mfma(const vu4x (&a)[TI][NP], const vu4x (&b)[TJ][NP], v16f (&acc)[TI][TJ]) {
  constexpr int NT = NP == 3 ? 6 : 3;
  // NP == 3: a_lo b_hi, a_hi b_lo, a_mid b_mid, a_mid b_hi, a_hi b_mid, a_hi b_hi;  NP == 2: a_lo b_hi, a_hi b_lo, a_hi b_hi
  constexpr int PA[6] = {NP == 3 ? 2 : 1, 0, NP == 3 ? 1 : 0, 1, 0, 0};
  constexpr int PB[6] = {0, NP == 3 ? 2 : 1, NP == 3 ? 1 : 0, 0, 1, 0};
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
      for (int ti = 0; ti < TI; ++ti) {
        const v16f zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const v16f c = (FIRST && t == 0) ? zero : acc[ti][tj];
        if constexpr (NP == 3)
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x3bf8, a[ti][PA[t]]),
                                                                __builtin_bit_cast(x3bf8, b[tj][PB[t]]), c, 0, 0, 0);
        else
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(x2h8, a[ti][PA[t]]),
                                                               __builtin_bit_cast(x2h8, b[tj][PB[t]]), c, 0, 0, 0);
      }
}

// ---- C[M x N] = A[M x K] W[N][K]^T as six bf16 MFMA terms (RNB_VARIANT_X3; the albedo network's GEMMs) -------------
// Same tiling and epilogues as gemm_rows_kernel (128 x BN output tile, 4 waves of 64 x BN/2), but the 16-k staging
// tiles are split into hi / mid / lo bf16 planes on their way into LDS (once per workgroup: every staged fp32 value
// is split by the thread that loaded it), and the waves multiply plane fragments: lane (row i, half h) reads 16 bytes
// = k 8h .. 8h + 7 of its row.  Plane tile: [rows][48 bytes] (16 bf16 + pad: conflict-free ds_read_b128).
constexpr int XK = 16;   // k per staging tile = one MFMA k-step
constexpr int XP = 48;   // bytes per row of a plane tile

typedef unsigned vu2x __attribute__((ext_vector_type(2)));
__device__ inline void x3_split4(const vf4& x, vu2x& hi, vu2x& mid, vu2x& lo) {
  const float v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float a = v[2 * p], b = v[2 * p + 1];
    unsigned uh = x3_pack2(a, b);
    asm("" : "+v"(uh));
    const float ra = a - __builtin_bit_cast(float, uh << 16);
    const float rb = __builtin_fmaf(__builtin_bit_cast(float, uh & 0xffff0000u), -1.f, b);
    unsigned um = x3_pack2(ra, rb);
    asm("" : "+v"(um));
    const float sa = ra - __builtin_bit_cast(float, um << 16);
    const float sb = __builtin_fmaf(__builtin_bit_cast(float, um & 0xffff0000u), -1.f, rb);
    hi[p] = uh;
    mid[p] = um;
    lo[p] = x3_pack2(sa, sb);
  }
}
__device__ inline void x2h_split4(const vf4& x, vu2x& hi, vu2x& lo) {   // x already scaled
  const float v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const unsigned uh = x2h_pack2(v[2 * p], v[2 * p + 1]);
    hi[p] = uh;
    lo[p] = x2h_pack2(x2h_resid_lo(v[2 * p], uh), x2h_resid_hi(v[2 * p + 1], uh));
  }
}
// ROWS x 16 k of a k-contiguous source -> ROWS / 64 float4 per thread (row idx >> 2, k quad idx & 3).  Buffer loads:
// the thread's (row, k quad) offset is loop-invariant (one VGPR per float4), the k offset of the tile is scalar.
template <int ROWS, bool GUARD>
__device__ inline void x3_rows_offsets(int ld, int r0, int rmax, int tid, unsigned (&off)[ROWS / 64], bool (&ok)[ROWS / 64]) {
#pragma unroll
  for (int i = 0; i < ROWS / 64; ++i) {
    const int idx = tid + 256 * i;
    const int r = idx >> 2, c4 = idx & 3;
    ok[i] = !GUARD || r0 + r < rmax;
    const int rr = ok[i] ? r0 + r : rmax - 1;   // GUARD: a clamped (valid) row, selected away below
    off[i] = ((unsigned)rr * (unsigned)ld + (unsigned)c4 * 4u) * 4u;
  }
}
template <int ROWS, bool GUARD>
__device__ inline void x3_load_rows(BufRsrc rs, const unsigned (&off)[ROWS / 64], const bool (&ok)[ROWS / 64], int k0,
                                    vf4 (&v)[ROWS / 64]) {
#pragma unroll
  for (int i = 0; i < ROWS / 64; ++i) {
    const vf4 t = __builtin_bit_cast(vf4, __builtin_amdgcn_raw_buffer_load_b128(rs, off[i], (unsigned)k0 * 4u, 0));
    if constexpr (!GUARD) v[i] = t;
    else v[i] = make_vf4(ok[i] ? t.x : 0.f, ok[i] ? t.y : 0.f, ok[i] ? t.z : 0.f, ok[i] ? t.w : 0.f);
  }
}
template <int ROWS>
__device__ inline void x3_store_rows(char* __restrict__ P, int tid, const vf4 (&v)[ROWS / 64]) {
#pragma unroll
  for (int i = 0; i < ROWS / 64; ++i) {
    const int idx = tid + 256 * i;
    const int r = idx >> 2, c4 = idx & 3;
    vu2x hi, mid, lo;
    x3_split4(v[i], hi, mid, lo);
    char* w = P + r * XP + c4 * 8;
    *reinterpret_cast<vu2x*>(w) = hi;
    *reinterpret_cast<vu2x*>(w + ROWS * XP) = mid;
    *reinterpret_cast<vu2x*>(w + 2 * ROWS * XP) = lo;
  }
}

template <int BN, bool GUARD, class Epi>
__global__ __launch_bounds__(256, 2) void gemm_rows_x3_kernel(const float* __restrict__ A, int lda,
                                                              const float* __restrict__ W, int ldw, int N, int K, Epi epi) {
  constexpr int TN = BN / 64;
  __shared__ __attribute__((aligned(16))) char smem[3 * (BM + BN) * XP];
  char* Ap = smem;
  char* Bp = smem + 3 * BM * XP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  const int m_blk = blockIdx.x * BM, n_blk = blockIdx.y * BN;
  unsigned mask = 0;
#pragma unroll
  for (int tj = 0; tj < TN; ++tj)
    if (n_blk + wn * (BN / 2) + tj * 32 < N) mask |= 1u << tj;
  const int i = lane & 31, h = lane >> 5;
  const char* fa = Ap + (wm * 64 + i) * XP + h * 16;
  const char* fb = Bp + (wn * (BN / 2) + i) * XP + h * 16;

  v16f acc[2][TN];
  zero_acc<TN>(acc);
  vf4 ra[BM / 64], rb[BN / 64];
  const int nk = K / XK;
  // resources based at the tile's first row (32-bit offsets stay inside the tile)
  const BufRsrc rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A + (size_t)m_blk * lda), 0, 0xfffffffc, 0x00020000);
  const BufRsrc rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W + (size_t)n_blk * ldw), 0, 0xfffffffc, 0x00020000);
  unsigned oa[BM / 64], ob[BN / 64];
  bool ka[BM / 64], kb[BN / 64];
  x3_rows_offsets<BM, false>(lda, 0, 0, tid, oa, ka);
  x3_rows_offsets<BN, GUARD>(ldw, 0, N - n_blk, tid, ob, kb);
  x3_load_rows<BM, false>(rsA, oa, ka, 0, ra);
  x3_load_rows<BN, GUARD>(rsW, ob, kb, 0, rb);
  for (int kt = 0; kt < nk; ++kt) {
    x3_store_rows<BM>(Ap, tid, ra);
    x3_store_rows<BN>(Bp, tid, rb);
    lds_barrier();
    {
      const int k0 = min(kt + 1, nk - 1) * XK;   // past the end: a harmless re-load
      x3_load_rows<BM, false>(rsA, oa, ka, k0, ra);
      x3_load_rows<BN, GUARD>(rsW, ob, kb, k0, rb);
    }
    vu4x a[2][3];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) a[ti][pl] = *reinterpret_cast<const vu4x*>(fa + pl * BM * XP + ti * 32 * XP);
#pragma unroll
    for (int tj = 0; tj < TN; ++tj) {
      if (GUARD && !((mask >> tj) & 1u)) continue;
      vu4x b[3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) b[pl] = *reinterpret_cast<const vu4x*>(fb + pl * BN * XP + tj * 32 * XP);
      constexpr int PA[6] = {2, 0, 1, 1, 0, 0};   // small terms first (x3_mfma)
      constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x3bf8, a[ti][PA[t]]),
                                                                __builtin_bit_cast(x3bf8, b[PB[t]]), acc[ti][tj], 0, 0, 0);
    }
    lds_barrier();
  }
  static_assert(4 * 16 * (32 * TN + 4) * 4 <= 3 * (BM + BN) * XP, "epilogue strips must fit in the staging LDS");
  run_epilogue<TN, Epi>(acc, reinterpret_cast<float*>(smem) + wave * 16 * (32 * TN + 4), m_blk + wm * 64,
                        n_blk + wn * (BN / 2), lane, mask, epi);
}

// ---- the same product with the WEIGHTS TAKEN FROM THE SPLIT MIRROR ("x3m"; the albedo network's GEMMs) -----------------
// gemm_rows_x3_kernel splits both operands on their way into LDS — the weight tile again in every one of the M / 128
// workgroups — behind two barriers per 16-k step.  Here only the activations are staged: one float4 per thread and step,
// split once, into one of two plane tiles [3][128][48 B] (one barrier per step; the split of step s + 1 rides beside the
// MFMAs of step s); the weight fragments come straight from the fragment-ordered mirror that rnb_weightnorm_fwd wrote
// (x3_pack_weights; one contiguous 1 KB per load, as in the fused sweeps), two steps ahead in registers.  One 8-wave
// workgroup per 128 rows; wave w owns ALL 128 rows x the column tiles w and (TJ == 2) w + 8 — every weight fragment is
// fetched once per workgroup, every activation split once.  N <= 32 * 8 * TJ, N % 32 == 0, K % 32 == 0.
// amax != nullptr: max |acc| over the rows below m_real is left there (an upper bound of the epilogue's masked outputs)
template <int TJ, class Epi>
__global__ __launch_bounds__(512, 1) void gemm_rows_x3m_kernel(const float* __restrict__ A, int lda,
                                                               const x3raw* __restrict__ W3, int N, int K, Epi epi,
                                                               unsigned* amax = nullptr, long long m_real = 0) {
  constexpr int NP = 3;   // (an fp16 two-plane form of this kernel existed in round 4; the fused albedo kernels replaced it)
  constexpr int ROWS = 128;
  constexpr int PLB = ROWS * XP;              // bytes of one plane
  constexpr int BUFB = NP * PLB;              // one staging buffer (three planes: 18,432 B)
  constexpr int STRIP = 16 * (32 + 4) * 4;    // epilogue strip of one wave (one 32-column tile at a time)
  __shared__ __attribute__((aligned(16))) char smem[2 * BUFB > 8 * STRIP ? 2 * BUFB : 8 * STRIP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id();
  const int m_blk = blockIdx.x * ROWS;
  const int nks = K >> 4;   // even
  int nt[TJ];
  bool on[TJ];
#pragma unroll
  for (int tj = 0; tj < TJ; ++tj) { nt[tj] = wave + 8 * tj; on[tj] = nt[tj] * 32 < N; }
  // staging role: row tid >> 2, k quad tid & 3 of every 16-k step
  const int sr = tid >> 2, sc = tid & 3;
  const BufRsrc rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A + (size_t)m_blk * lda), 0, 0xfffffffc, 0x00020000);
  const unsigned aoff = ((unsigned)sr * (unsigned)lda + (unsigned)sc * 4u) * 4u;
  char* const swr = smem + sr * XP + sc * 8;
  const int i = lane & 31, h = lane >> 5;
  const char* const fa = smem + i * XP + h * 16;
  const BufRsrc rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<x3raw*>(W3), 0, 0x7ffffff0, 0x00020000);
  const unsigned boff = (unsigned)lane * 16u;
  auto load_b = [&](int ks, vu4x (&b)[TJ][NP]) {
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      const unsigned soff = (unsigned)((on[tj] ? nt[tj] : 0) * nks + ks) * (NP * 1024u);
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        b[tj][pl] = __builtin_bit_cast(vu4x, __builtin_amdgcn_raw_buffer_load_b128(rsW, boff, soff + pl * 1024, 0));
    }
  };
  auto load_a = [&](int ks) {
    return __builtin_bit_cast(vf4, __builtin_amdgcn_raw_buffer_load_b128(rsA, aoff, (unsigned)ks * 64u, RNB_AUX_LD));
  };
  auto stage = [&](const vf4& x, int buf) {
    char* w = swr + buf * BUFB;
    vu2x hi, mid, lo;
    x3_split4(x, hi, mid, lo);
    *reinterpret_cast<vu2x*>(w) = hi;
    *reinterpret_cast<vu2x*>(w + PLB) = mid;
    *reinterpret_cast<vu2x*>(w + 2 * PLB) = lo;
  };
  v16f acc[4][TJ];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;
  vu4x b0[TJ][NP], b1[TJ][NP];
  load_b(0, b0);
  load_b(1, b1);
  vf4 x = load_a(0);
  stage(x, 0);
  x = load_a(1);
  auto step = [&](int ks, vu4x (&b)[TJ][NP]) {
    // buffer ks & 1 holds step ks (written before the barrier); buffer (ks + 1) & 1 was read in step ks - 1: free
    lds_barrier();
    stage(x, (ks + 1) & 1);                        // step ks + 1 (past the end: a harmless re-stage of the last step)
    x = load_a(min(ks + 2, nks - 1));
    const char* f = fa + (ks & 1) * BUFB;
    vu4x a[4][NP];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) a[ti][pl] = *reinterpret_cast<const vu4x*>(f + pl * PLB + ti * 32 * XP);
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0};   // small terms first (x3_mfma)
    constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      if (TJ == 2 && tj == 1 && !on[1]) continue;   // (wave-uniform)
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x3bf8, a[ti][PA[t]]),
                                                                __builtin_bit_cast(x3bf8, b[tj][PB[t]]), acc[ti][tj], 0, 0, 0);
    }
    load_b(min(ks + 2, nks - 1), b);
  };
  for (int ks = 0; ks < nks; ks += 2) {
    step(ks, b0);
    step(ks + 1, b1);
  }
  __syncthreads();   // the staging buffers become the epilogue strips
  if (amax != nullptr) {   // (workgroup-uniform)  the eight waves' maxima meet in LDS: one atomic per workgroup
    __shared__ float wmx[8];
    const long long left = m_real - m_blk;
    float m = 0.f;
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      if (!on[tj]) continue;
      v16f t[4][1];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) t[ti][0] = acc[ti][tj];
      m = fmaxf(m, acc_absmax<4, 1>(t, lane, left >= ROWS ? ROWS : (int)(left < 0 ? 0 : left)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) wmx[wave] = m;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 8; ++w) m = fmaxf(m, wmx[w]);
      const unsigned b = __builtin_bit_cast(unsigned, m);
      if (b > __atomic_load_n(amax, __ATOMIC_RELAXED)) atomicMax(amax, b);
    }
  }
  float* strip = reinterpret_cast<float*>(smem + wave * STRIP);
#pragma unroll
  for (int tj = 0; tj < TJ; ++tj) {
    if (!on[tj]) continue;
    v16f t[4][1];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) t[ti][0] = acc[ti][tj];
    run_epilogue<1, Epi, 4>(t, strip, m_blk, nt[tj] * 32, lane, 1u, epi);
  }
}

// ---- 64-point row tiles through LDS ------------------------------------------------------------------
// The per-point kernels below compute (or consume) W consecutive columns of one matrix row per lane.
// Touching global memory in that shape makes every access instruction hit 64 different rows; instead one
// wave stages its 64 rows x W columns in LDS (pitch W + 1: conflict-free both ways) and moves them with
// 16 bytes per lane along the rows; the last W % 4 columns of a row move as single floats (an albedo input block
// behind a feature width that is no multiple of 4: Cinp - F).  ld % 4 == 0; col0 % 4 == 0 keeps the 16-byte accesses
// aligned (they are dword-aligned otherwise); one wave per workgroup.
__device__ inline void tile_store64(float* __restrict__ dst, int ld, int64_t r0, int col0, int W,
                                    const float* __restrict__ tile, int lane) {
  const int g = W >> 2;   // 16-byte groups per row
  for (int idx = lane; idx < 64 * g; idx += 64) {
    const int p = idx / g, c = (idx - p * g) * 4;
    const float* t = tile + p * (W + 1) + c;
    *reinterpret_cast<vf4*>(dst + (r0 + p) * ld + col0 + c) = make_vf4(t[0], t[1], t[2], t[3]);
  }
  if (const int rest = W & 3) {
    for (int idx = lane; idx < 64 * rest; idx += 64) {
      const int p = idx / rest, c = (W - rest) + (idx - p * rest);
      dst[(r0 + p) * ld + col0 + c] = tile[p * (W + 1) + c];
    }
  }
}
__device__ inline void tile_load64(const float* __restrict__ src, int ld, int64_t r0, int col0, int W,
                                   float* __restrict__ tile, int lane) {
  const int g = W >> 2;
  for (int idx = lane; idx < 64 * g; idx += 64) {
    const int p = idx / g, c = (idx - p * g) * 4;
    const vf4 v = *reinterpret_cast<const vf4*>(src + (r0 + p) * ld + col0 + c);
    float* t = tile + p * (W + 1) + c;
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
  }
  if (const int rest = W & 3) {
    for (int idx = lane; idx < 64 * rest; idx += 64) {
      const int p = idx / rest, c = (W - rest) + (idx - p * rest);
      tile[p * (W + 1) + c] = src[(r0 + p) * ld + col0 + c];
    }
  }
}

// ---- activation helpers ----------------------------------------------------------------------------
// nn.Softplus(beta=100) with PyTorch's threshold 20 (models/fields.py:80)
__device__ inline float softplus100(float z) {
  const float t = z * 100.f;
  return t > 20.f ? z : log1pf(expf(t)) * 0.01f;
}
// softplus and its derivative in one go: a = softplus_100(z), D = sigmoid(100 z).
// On gfx950 the fp32 MFMA and ordinary vector instructions exclude each other on a SIMD, so this function is
// paid for in matrix time: it is written for instruction count (16 VALU + 3 transcendentals per element,
// most of them packable two elements at a time — see the vf2 overload).
//   w = exp(-|t|), t = 100 z        (never overflows; no range clamp needed)
//   a = max(z, 0) + log1p(w) / 100  (for t > 20 the second term is below half an ulp of z: a == z exactly,
//                                    PyTorch's threshold branch, models/fields.py:80)
//   D = 1 / (1 + w)  (t >= 0)   |   w / (1 + w)  (t < 0)        (== 1 exactly for t > 20)
// exp through the hardware exp2 with the rounding error of the product -|t| log2(e) fed back to first order;
// log1p(w) = log(u) + (w - (u - 1)) / u with u = fl(1 + w) (rounding-compensated, hardware log2 and rcp).
__device__ inline void softplus_aD(float z, float& a, float& D) {
  constexpr float L2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;
  const float t = z * 100.f;
  const float nt = -fabsf(t);
  const float p = nt * L2E;
  const float q = __builtin_fmaf(nt, L2E, -p);
  const float w0 = __builtin_amdgcn_exp2f(p);
  const float w = __builtin_fmaf(w0, q * LN2, w0);
  const float u = 1.f + w;
  const float r = __builtin_amdgcn_rcpf(u);
  const float lg = __builtin_amdgcn_logf(u);
  const float l1p = __builtin_fmaf(lg, LN2, (w - (u - 1.f)) * r);
  a = __builtin_fmaf(l1p, 0.01f, fmaxf(z, 0.f));
  D = t >= 0.f ? r : w * r;
}
// two elements at a time: the multiplies / adds / fmas become v_pk_*_f32 (one issue slot for both)
__device__ inline void softplus_aD(vf2 z, vf2& a, vf2& D) {
  constexpr float L2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;
  const vf2 t = z * 100.f;
  const vf2 nt = {-fabsf(t.x), -fabsf(t.y)};
  const vf2 p = nt * L2E;
  const vf2 q = __builtin_elementwise_fma(nt, vf2{L2E, L2E}, -p);
  const vf2 w0 = {__builtin_amdgcn_exp2f(p.x), __builtin_amdgcn_exp2f(p.y)};
  const vf2 w = __builtin_elementwise_fma(w0, q * LN2, w0);
  const vf2 u = w + 1.f;
  const vf2 r = {__builtin_amdgcn_rcpf(u.x), __builtin_amdgcn_rcpf(u.y)};
  const vf2 lg = {__builtin_amdgcn_logf(u.x), __builtin_amdgcn_logf(u.y)};
  const vf2 l1p = __builtin_elementwise_fma(lg, vf2{LN2, LN2}, (w - (u - 1.f)) * r);
  const vf2 zp = {fmaxf(z.x, 0.f), fmaxf(z.y, 0.f)};
  a = __builtin_elementwise_fma(l1p, vf2{0.01f, 0.01f}, zp);
  const vf2 wr = w * r;
  D = vf2{t.x >= 0.f ? r.x : wr.x, t.y >= 0.f ? r.y : wr.y};
}
// a alone (forward-only evaluations, e.g. the sampling passes): no reciprocal — the compensation term
// (w - (u - 1)) / u is at most half an ulp of u, so 1 / u ~ 1 - w inside it changes a by < eps w / 2.
__device__ inline vf2 softplus_a(vf2 z) {
  constexpr float L2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;
  const vf2 t = z * 100.f;
  const vf2 nt = {-fabsf(t.x), -fabsf(t.y)};
  const vf2 p = nt * L2E;
  const vf2 q = __builtin_elementwise_fma(nt, vf2{L2E, L2E}, -p);
  const vf2 w0 = {__builtin_amdgcn_exp2f(p.x), __builtin_amdgcn_exp2f(p.y)};
  const vf2 w = __builtin_elementwise_fma(w0, q * LN2, w0);
  const vf2 u = w + 1.f;
  const vf2 lg = {__builtin_amdgcn_logf(u.x), __builtin_amdgcn_logf(u.y)};
  const vf2 d = w - (u - 1.f);
  const vf2 l1p = __builtin_elementwise_fma(lg, vf2{LN2, LN2}, __builtin_elementwise_fma(-d, w, d));
  const vf2 zp = {fmaxf(z.x, 0.f), fmaxf(z.y, 0.f)};
  return __builtin_elementwise_fma(l1p, vf2{0.01f, 0.01f}, zp);
}
// The same two functions on scalars, for the x3 kernels: there the epilogue of one wave runs beside the other wave's bf16
// MFMAs, where packed fp32 instructions are an anti-lever (MI355X_MICROARCH.md: a v_pk_* costs ~13 cycles more than the
// two scalar instructions it replaces).  Bit-identical results (same operations, element-wise).
__device__ inline float softplus_a(float z) {
  constexpr float L2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;
  const float t = z * 100.f;
  const float nt = -fabsf(t);
  const float p = nt * L2E;
  const float q = __builtin_fmaf(nt, L2E, -p);
  const float w0 = __builtin_amdgcn_exp2f(p);
  const float w = __builtin_fmaf(w0, q * LN2, w0);
  const float u = w + 1.f;
  const float lg = __builtin_amdgcn_logf(u);
  const float d = w - (u - 1.f);
  const float l1p = __builtin_fmaf(lg, LN2, __builtin_fmaf(-d, w, d));
  return __builtin_fmaf(l1p, 0.01f, fmaxf(z, 0.f));
}
template <bool SCALAR>
__device__ inline vf2 softplus_a_sel(vf2 z) {
  if constexpr (SCALAR) return vf2{softplus_a(z.x), softplus_a(z.y)};
  else return softplus_a(z);
}
template <bool SCALAR>
__device__ inline void softplus_aD_sel(vf2 z, vf2& a, vf2& D) {
  if constexpr (SCALAR) {
    float a0, a1, D0, D1;
    softplus_aD(z.x, a0, D0);
    softplus_aD(z.y, a1, D1);
    a = vf2{a0, a1};
    D = vf2{D0, D1};
  }
  else softplus_aD(z, a, D);
}
// D = d softplus / dz = sigmoid(100 z) expressed through a = softplus(z):  D = 1 - exp(-100 a)
// (exactly 1 above the threshold, where a == z); E = 1 - D, and softplus'' = 100 D E.
__device__ inline void softplus_DE(float a, float& D, float& E) {
  const float t = a * 100.f;
  if (t > 20.f) { D = 1.f; E = 0.f; }
  else { D = -expm1f(-t); E = expf(-t); }
}
__device__ inline float softplus_D(float a) {
  const float t = a * 100.f;
  return t > 20.f ? 1.f : -expm1f(-t);
}

}  // namespace rnb
