// RNB_VARIANT_BF16 — BASELINE config 5: the sweeps of the 256-wide SDF network with bf16 operands on
// v_mfma_f32_32x32x16_bf16 and fp32 accumulators.  Same mathematics as fused.hip / fused_bwd.hip (oracle/explicit.py is
// the statement); what changes is the arithmetic of the matrix products and the format of the per-point saved state.
// This header is what the route's three units share: the types, the matrix loop and the K8 access helpers.
//
//   bf16_sweeps.hip  bf_forward_kernel   positional encoding + F sweep (+ sdf head, + feature head)   models/fields.py:82-104
//                    bf_reverse_kernel   R : reverse-mode normal                                      models/fields.py:114-127
//                    bf_ra_kernel        RA: adjoint of R
//                    bf_fb_kernel        FB: backward of F
//                    bf_pack_kernel      fp32 packed weights -> the bf16 mirror in MFMA-fragment order
//   bf16_color.hip   bf_color_{fwd,bwd,out_bwd}_kernel   the albedo network (where bf16_color_supported)
//   bf16_dw.hip      bf_dw_kernel        dW_l = gz_l^T u_l + zb_l^T in_l for all layers (grouped launch, split over points)
//                    bf_dw_reduce_kernel ordered reduction of its slabs (deterministic variant)
//                    bf_sdf_head_bwd_kernel  gradient of the sdf-head row
//
// At 1/16 of the fp32 matrix time these sweeps are bound by the HBM traffic of the saved state, not by the matrix
// cores.  Saved state is therefore bf16, in ONE layout that serves every consumer without a transpose:
// "K8" = [points / 8][columns][8 points].  (1) An accumulator tile of v_mfma_f32_32x32x16_bf16 holds, per lane, one
// column and rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5): registers 4g .. 4g+3 are four consecutive points of one
// column = 8 contiguous bytes of a K8 matrix, and the 64 lanes of one store instruction cover 512 contiguous bytes.
// (2) The weight-gradient product sums over points: its MFMA operands are "8 consecutive points of one column" for
// both X^T and Y — exactly one 16-byte K8 unit per lane, coalesced, no LDS, no transposed reads.
// Activations inside a sweep stay in LDS as row-major bf16 [point][256] (pitch 264: conflict-free ds_read_b128 of the
// A fragments); weights stream from L2 as bf16 rows of the mirror that rnb_weightnorm_fwd appends to the packed buffer.
// fp32 master weights, fp32 gradients (split-K partial sums leave through fp32 atomics or ordered slabs), fp32
// epilogue math; only what enters an MFMA or goes to HBM per point is rounded to bf16 (round-to-nearest-even).
#pragma once
#include "fused_common.hip.h"

namespace rnb {

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef unsigned vu4 __attribute__((ext_vector_type(4)));
typedef unsigned short bfraw;   // storage type of one bf16 (no arithmetic on it)

constexpr int BP = 264;    // LDS pitch (bf16 elements) of an activation row: 528 bytes
constexpr int BT = 64;     // points per workgroup
// Every sweep kernel is templated on TI = 32-row MFMA tiles per wave.  TI = 2: 4 waves per workgroup, each all 64 rows x
// 64 columns.  TI = 1: 8 waves, wave = (row half, column group), 32 rows x 64 columns each: half the accumulator and
// prefetch registers (<= 128), so two workgroups per CU are 4 waves per SIMD instead of 2.  (Kept as an A/B variant:
// although the TI = 2 sweeps are parked 46-69 % of the time (SQ_WAIT_ANY), TI = 1 is slower — see bf_ti below.)
template <int TI> struct BfCfg { static constexpr int NW = 8 / TI; static constexpr int NT = 64 * NW; };

__device__ inline unsigned pack2(float a, float b) {
  bf2 p = {(__bf16)a, (__bf16)b};   // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
  return __builtin_bit_cast(unsigned, p);
}
// A value the optimiser cannot see through: address arithmetic derived from it is redone where it is used instead of
// being hoisted out of the layer loop (loop-invariant per-lane offsets of ~40 loads and stores, kept live across the
// matrix loop, were what spilled in the sweeps with two epilogue operand tiles).
__device__ inline int opaque(int v) { asm volatile("" : "+v"(v)); return v; }
__device__ inline bfraw to_bf(float a) { return __builtin_bit_cast(bfraw, (__bf16)a); }
__device__ inline float bf_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ inline float bf_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }
__device__ inline float bf_f(bfraw v) { return __builtin_bit_cast(float, (unsigned)v << 16); }

// element offset of (row, col) in a K8 matrix with C columns
__device__ inline size_t k8(int64_t row, int col, int C) { return ((size_t)(row >> 3) * C + col) * 8 + (row & 7); }

// ---- matrix loop ------------------------------------------------------------------------------------------
// acc[ti][tj] = X[64 rows][K] * W[n0 + 32 tj + .][K]^T for one wave (rows: all 64 of the tile), K a multiple of 64.
// X: LDS, row-major bf16, pitch BP.  W: global bf16 [N][K] row-major; lane (i, h) streams 16 bytes (k = 8h .. 8h+7 of
// the 16-k step) of weight row n0 + 32 tj + i per step.  Weight fragments run one 64-k block ahead in a second
// register set (two alternating sets, no copies).
// KS = 16-k steps per prefetched weight block: 4 (two register sets of 32) at TI = 2, 2 (two sets of 16) at TI = 1,
// where four resident waves per SIMD cover the L2 latency instead of a deeper per-wave prefetch.
// Weight matrices in the bf16 mirror are stored in MFMA-FRAGMENT ORDER (bf16_pack_weights): for W [N][K], fragment
// (nt, ks) = rows 32 nt .. +32, k = 16 ks .. +16 is 64 consecutive 16-byte units, unit (h, c) = W[32 nt + c][16 ks + 8 h .. +8].
// One B-fragment load of a wave is then ONE contiguous 1 KB read (8 cache lines).  Row-major weights make the same
// load touch 32 lines (32 bytes of each of 32 rows) — at 8 loads per 16 MFMAs that kept the L1 tag pipeline, not the
// matrix cores, busy: the sweeps ran at 14 % of the bf16 MFMA rate.
// (buffer loads: lane * 16 in one VGPR, the fragment's offset in the scalar operand, the step in the immediate — no
// vector address arithmetic in front of the loads)
template <int KS>
__device__ inline void bf_load_b(const bfraw* __restrict__ W, int K, int n0, int Q, int lane, vu4 (&b)[KS][2]) {
  const int nks = K >> 4;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bfraw*>(W), 0, 0x4000000, 0x00020000);
  const unsigned voff = (unsigned)lane * 16u;
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const unsigned soff = (unsigned)(((n0 >> 5) + tj) * nks + Q * KS) * 1024u;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      b[s][tj] = __builtin_bit_cast(vu4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff + s * 1024, 0));
  }
}
// One 16 KS-k block: the A fragments of step s + 1 are read from LDS while the MFMAs of step s run (explicit rotation +
// a scheduling fence per step: left alone, hipcc parks every ds_read right in front of its MFMAs and waits for it).
template <int TI, int KS, int PITCH>
__device__ inline void bf_mma_block(const bfraw* __restrict__ X, int Q, int lane, const vu4 (&b)[KS][2], v16f (&acc)[TI][2]) {
  const int i = lane & 31, h = lane >> 5;
  const bfraw* xp = X + i * PITCH + Q * (16 * KS) + h * 8;
  vu4 a[2][TI];
#pragma unroll
  for (int ti = 0; ti < TI; ++ti) a[0][ti] = *reinterpret_cast<const vu4*>(xp + ti * 32 * PITCH);
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (s + 1 < KS) {
#pragma unroll
      for (int ti = 0; ti < TI; ++ti) a[(s + 1) & 1][ti] = *reinterpret_cast<const vu4*>(xp + ti * 32 * PITCH + (s + 1) * 16);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int ti = 0; ti < TI; ++ti)
        acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, a[s & 1][ti]), __builtin_bit_cast(bf8, b[s][tj]),
                                                              acc[ti][tj], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <int TI>
__device__ inline void bf_zero(v16f (&acc)[TI][2]) {
#pragma unroll
  for (int a = 0; a < TI; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}
// X points at the first of the wave's 32 TI rows.
// `pre` holds weight block 0 of THIS product, requested by the previous call (`Wnext` / `Knext`: the product that
// follows; its block 0 is requested here as soon as this product's last block is in flight, so that it lands during
// the epilogue instead of costing an exposed L2 round trip at the top of every layer).  The block loop is unrolled for
// the compile-time block count NQ (K = 64 NQ / (4 / KS)): two alternating register sets, no copies for even NQ.
template <int TI, int PITCH = BP, int KSV = (TI == 1 ? 2 : 4)>
struct BfMma {
  static constexpr int KS = KSV;
  vu4 pre[KS][2];
  __device__ inline void request(const bfraw* __restrict__ W, int K, int n0, int lane) { bf_load_b<KS>(W, K, n0, 0, lane, pre); }
  template <int NQ>
  __device__ inline void run_fixed(const bfraw* __restrict__ X, const bfraw* __restrict__ W, int K, int n0, int lane,
                                   v16f (&acc)[TI][2], const bfraw* __restrict__ Wnext, int Knext, int n0next) {
    bf_zero<TI>(acc);
    vu4 alt[KS][2];
    __builtin_amdgcn_s_setprio(1);   // (the matrix loop outranks the other workgroup's epilogue on this SIMD)
#pragma unroll
    for (int Q = 0; Q < NQ; ++Q) {
      // request the block after this one into the set that is not being multiplied
      if (Q + 1 < NQ) {
        if (Q & 1) bf_load_b<KS>(W, K, n0, Q + 1, lane, pre); else bf_load_b<KS>(W, K, n0, Q + 1, lane, alt);
      } else if (Wnext) {
        if (Q & 1) bf_load_b<KS>(Wnext, Knext, n0next, 0, lane, pre); else bf_load_b<KS>(Wnext, Knext, n0next, 0, lane, alt);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (Q & 1) bf_mma_block<TI, KS, PITCH>(X, Q, lane, alt, acc); else bf_mma_block<TI, KS, PITCH>(X, Q, lane, pre, acc);
    }
    __builtin_amdgcn_s_setprio(0);
    if ((NQ & 1) && Wnext) {   // odd block count: the next product's block 0 sits in `alt`
#pragma unroll
      for (int s = 0; s < KS; ++s) { pre[s][0] = alt[s][0]; pre[s][1] = alt[s][1]; }
    }
  }
  // K is one of 64 (PE input), 256 (hidden) or 320 (the albedo net's input): the call sites know which
  template <int KK>
  __device__ inline void run(const bfraw* __restrict__ X, const bfraw* __restrict__ W, int n0, int lane, v16f (&acc)[TI][2],
                             const bfraw* __restrict__ Wnext, int Knext, int n0next) {
    run_fixed<KK / (16 * KS)>(X, W, KK, n0, lane, acc, Wnext, Knext, n0next);
  }
};
template <int TI, int PITCH = BP>
__device__ inline void bf_layer_mma(const bfraw* __restrict__ X, const bfraw* __restrict__ W, int K, int n0, int lane,
                                    v16f (&acc)[TI][2]) {
  BfMma<TI, PITCH> m;
  m.request(W, K, n0, lane);
  if (K == 256) m.template run<256>(X, W, n0, lane, acc, nullptr, 0, 0);
  else if (K == 64) m.template run<64>(X, W, n0, lane, acc, nullptr, 0, 0);
  else m.template run<320>(X, W, n0, lane, acc, nullptr, 0, 0);
}

// ---- accumulator-layout access to K8 matrices -------------------------------------------------------------------
// One "quad" = registers 4g .. 4g+3 of one 32 x 32 accumulator tile = points 8g + 4h .. +3 of one column = 8 bytes.
// Buffer accesses: resource based at the wave's first K8 block row (row0 is wave-uniform), the lane's (column, half)
// offset in ONE VGPR, the quad's block row in the scalar operand — no 64-bit vector address per quad (the epilogues of
// these sweeps are what the vector port is busy with).
struct Quad { float v[4]; };
__device__ inline __amdgpu_buffer_rsrc_t k8_rsrc(const bfraw* base, int64_t row0, int C) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<bfraw*>(base) + (size_t)(row0 >> 3) * C * 8, 0, 0x7ffffff0, 0x00020000);
}
__device__ inline Quad k8_load_quad(const bfraw* __restrict__ base, int64_t row0, int ti, int g, int col, int h) {
  const vu2 u = __builtin_bit_cast(vu2, __builtin_amdgcn_raw_buffer_load_b64(k8_rsrc(base, row0, FH), (unsigned)(col * 16 + 8 * h),
                                                                               (unsigned)((ti * 4 + g) * FH * 16), RNB_AUX_LD));
  return Quad{{bf_lo(u.x), bf_hi(u.x), bf_lo(u.y), bf_hi(u.y)}};
}
__device__ inline void k8_store_quad(bfraw* __restrict__ base, int64_t row0, int ti, int g, int col, int h, float a, float b,
                                     float c, float d, int C = FH) {
  const vu2 u = {pack2(a, b), pack2(c, d)};
  __builtin_amdgcn_raw_buffer_store_b64(u, k8_rsrc(base, row0, C), (unsigned)(col * 16 + 8 * h), (unsigned)((ti * 4 + g) * C * 16), RNB_AUX_ST);
}
// 8 rows of one column of an LDS tile (row-major, pitch P) -> one 16-byte K8 unit
template <int P>
__device__ inline vu4 lds_gather8(const bfraw* __restrict__ X, int blk, int c) {
  bfraw v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = X[(blk * 8 + j) * P + c];
  return vu4{(unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16),
             (unsigned)v[4] | ((unsigned)v[5] << 16), (unsigned)v[6] | ((unsigned)v[7] << 16)};
}
// one 16-byte K8 unit -> 8 rows of one column of an LDS tile
template <int P>
__device__ inline void lds_scatter8(bfraw* __restrict__ X, int blk, int c, vu4 u) {
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) X[(blk * 8 + j) * P + c] = (bfraw)((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu));
}
// a whole [64 x 256] tile of a K8 matrix in accumulator layout (issued early, consumed after the matrix loop)
template <int TI> struct AuxBf { vu2 q[TI][2][4]; };
template <int TI>
__device__ inline void k8_prefetch(const bfraw* __restrict__ base, int64_t row0, int n0, int lane, AuxBf<TI>& t) {
  const int c = lane & 31, h = lane >> 5;
  const __amdgpu_buffer_rsrc_t rs = k8_rsrc(base, row0, FH);
#pragma unroll
  for (int ti = 0; ti < TI; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        t.q[ti][tj][g] = __builtin_bit_cast(vu2, __builtin_amdgcn_raw_buffer_load_b64(
            rs, (unsigned)((n0 + c) * 16 + 8 * h), (unsigned)((ti * 4 + g) * FH * 16 + tj * 512), RNB_AUX_LD));
}
template <int TI>
__device__ inline float aux_at(const AuxBf<TI>& t, int ti, int tj, int r) {
  const vu2 u = t.q[ti][tj][r >> 2];
  const unsigned w = (r & 2) ? u.y : u.x;
  return (r & 1) ? bf_hi(w) : bf_lo(w);
}

// softplus(beta = 100) and its derivative for bf16 consumers: hardware exp2 / log2 / rcp without the compensation
// terms of the fp32 path (their error, ~1e-7 relative, is far below half a bf16 ulp = 2e-3 relative)
__device__ inline void softplus_aD_fast(float z, float& a, float& D) {
  constexpr float L2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;
  const float t = z * 100.f;
  const float w = __builtin_amdgcn_exp2f(-fabsf(t) * L2E);
  const float u = 1.f + w;
  const float r = __builtin_amdgcn_rcpf(u);
  a = __builtin_fmaf(__builtin_amdgcn_logf(u), LN2 * 0.01f, fmaxf(z, 0.f));
  D = t >= 0.f ? r : w * r;
}

// Rows per workgroup of the one-thread-per-column reductions (bf_sdf_head_bwd_kernel, bf_color_out_bwd_kernel): 256 point
// slabs, ONE in the deterministic variant (a single add onto zero per address); whole 8-point K8 blocks.
inline int64_t bf_rows_per_slab(const Layout& L, int64_t M) {
  const int64_t slabs = (L.variant & RNB_VARIANT_DETERMINISTIC) ? 1 : 256;
  return ((M + slabs - 1) / slabs + 7) / 8 * 8;
}

}  // namespace rnb
