// Sparse SDF grid (rnb_sdf_grid_sparse_*): which bricks of the grid are evaluated, and what the others hold.
//
// A brick is a cube of bs^3 cells = (bs + 1)^3 samples; neighbours share their face samples.  The brick corners (the
// lattice) are evaluated first; bricks whose corners say "the surface may pass here" are listed (classify), listed bricks are
// evaluated by the forward sweeps in brick mode (GridGen, rnb_internal.h), every face of an evaluated brick whose samples
// are not all inside / all outside lists the brick behind it (grow), and in the end every sample no listed brick contains
// gets the clamped trilinear interpolant of its brick's corners (fill).  "Inside" is marching cubes' notion, value <=
// threshold with NaN outside (mcubes.hip).  Integer atomics only; the list is appended to through a device counter the host
// reads once per round.
#include "rnb_internal.h"

namespace rnb {

__device__ inline bool sg_inside(float v, float thr) { return v <= thr; }   // (NaN: outside)
__device__ inline int sg_state(const uint32_t* state, int b) { return (state[b >> 2] >> (8 * (b & 3))) & 0xff; }
// marks brick b as listed; true for the one caller that found it unlisted ("append once")
__device__ inline bool sg_claim(uint32_t* state, int b) {
  const uint32_t bit = 1u << (8 * (b & 3));
  return (atomicOr(state + (b >> 2), bit) & bit) == 0;
}

// ---- classify + compact: lattice -> seed flags -> brick list ---------------------------------------------------------
// One thread per brick.  A seed: a non-finite corner, corners on both sides of the threshold, or a corner closer to the
// threshold than seed_dist (= margin x half the brick's diagonal).  The seeds of a workgroup are compacted with a wave
// ballot + prefix and take their place in the list with ONE atomic add; the state bytes are written as whole words (lane 4k
// assembles the word of its four bricks from the ballot), so the word-wide integer or of the growth kernel finds them.
__global__ __launch_bounds__(256) void sparse_classify_kernel(SparseGeom sg, const float* __restrict__ lat,
                                                              uint32_t* __restrict__ state, int32_t* __restrict__ list,
                                                              unsigned long long* __restrict__ n_listed) {
  __shared__ int wcnt[4];
  __shared__ unsigned long long base;
  const int64_t nbr = (int64_t)sg.nb * sg.nb * sg.nb;
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool seed = false;
  if (b < nbr) {
    const int nl = sg.nl;
    const int bz = (int)(b % sg.nb), by = (int)((b / sg.nb) % sg.nb), bx = (int)(b / ((int64_t)sg.nb * sg.nb));
    int n_in = 0;
    bool bad = false;
    float dmin = __builtin_inff();
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float v = lat[((int64_t)(bx + (c >> 2)) * nl + by + ((c >> 1) & 1)) * nl + bz + (c & 1)];
      bad |= !(fabsf(v) < __builtin_inff());
      n_in += sg_inside(v, sg.thr) ? 1 : 0;
      dmin = fminf(dmin, fabsf(v - sg.thr));
    }
    seed = bad || (n_in != 0 && n_in != 8) || dmin < sg.seed_dist;
  }
  const unsigned long long m = __builtin_amdgcn_ballot_w64(seed);
  // state bytes of this wave's 64 bricks: lane 4k assembles word k (the grid is padded to whole words by the caller)
  if ((lane & 3) == 0 && (b >> 2) < (nbr + 3) / 4) {
    const unsigned nib = (unsigned)(m >> lane) & 0xfu;
    state[b >> 2] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
  }
  if (lane == 0) wcnt[wave] = __builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    base = tot ? atomicAdd(n_listed, (unsigned long long)tot) : 0ull;
  }
  __syncthreads();
  if (seed) {
    int off = __builtin_popcountll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) off += wcnt[w];
    list[base + off] = (int32_t)b;
  }
}

// ---- grow: the six faces of the bricks evaluated in the last round ------------------------------------------------------
// One workgroup per brick list[first + blockIdx.x]: every thread looks at a share of the six face layers in the volume and
// votes "has an inside sample" / "has an outside sample" per face (LDS integer or); a mixed face claims the brick behind it.
__global__ __launch_bounds__(256) void sparse_grow_kernel(SparseGeom sg, const float* __restrict__ vol, int64_t first,
                                                          uint32_t* __restrict__ state, int32_t* __restrict__ list,
                                                          unsigned long long* __restrict__ n_listed) {
  __shared__ unsigned votes;   // bit 2f: face f has an inside sample, bit 2f + 1: an outside one
  if (threadIdx.x == 0) votes = 0u;
  __syncthreads();
  const int b = list[first + blockIdx.x];
  const int nb = sg.nb, res = sg.res;
  const int bc[3] = {b / (nb * nb), (b / nb) % nb, b % nb};
  int lo[3], n[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    lo[d] = bc[d] * sg.bs;
    n[d] = min(lo[d] + sg.bs, res - 1) - lo[d] + 1;   // samples of the brick along d (a short last brick)
  }
  unsigned mine = 0u;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const int d = f >> 1, side = f & 1;
    if (side ? bc[d] + 1 >= nb : bc[d] == 0) continue;   // no brick behind this face
    const int da = d == 2 ? 1 : 2, db = d == 0 ? 1 : 0;   // fast / slow axis of the layer (fast = z whenever it can be)
    const int cnt = n[da] * n[db];
    for (int t = threadIdx.x; t < cnt; t += 256) {
      int i[3];
      i[d] = lo[d] + (side ? n[d] - 1 : 0);
      i[da] = lo[da] + t % n[da];
      i[db] = lo[db] + t / n[da];
      const float v = vol[((int64_t)i[0] * res + i[1]) * res + i[2]];
      mine |= (sg_inside(v, sg.thr) ? 1u : 2u) << (2 * f);
    }
  }
  if (mine) atomicOr(&votes, mine);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const unsigned v = votes;
  int fresh[6], nf = 0;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    if (((v >> (2 * f)) & 3u) != 3u) continue;
    const int d = f >> 1;
    const int stride = d == 0 ? nb * nb : (d == 1 ? nb : 1);
    const int nbr = b + ((f & 1) ? stride : -stride);
    if (sg_claim(state, nbr)) fresh[nf++] = nbr;
  }
  if (nf == 0) return;
  const unsigned long long at = atomicAdd(n_listed, (unsigned long long)nf);
  for (int k = 0; k < nf; ++k) list[at + k] = fresh[k];
}

// ---- fill: every sample no listed brick contains ------------------------------------------------------------------------
// One sample per thread and pass of a grid-stride loop, z fastest (coalesced stores).  The sample's owner is brick floor(i / bs) per axis (the last brick
// also owns the grid's last layer); a sample on a low face belongs to the bricks below as well, and if ANY brick that
// contains it is listed it holds an evaluated value and is left alone.  Otherwise the owner's eight corners are interpolated
// ((1 - t) a + t b per axis: exact at t = 0 and 1, so the interpolant is continuous across faces) and clamped to their
// minimum / maximum, which keeps the value on the corners' side of the threshold.
__global__ __launch_bounds__(256) void sparse_fill_kernel(SparseGeom sg, const float* __restrict__ lat,
                                                          const uint32_t* __restrict__ state, float* __restrict__ vol) {
  const int res = sg.res, nb = sg.nb, nl = sg.nl, bs = sg.bs;
  const int64_t n = (int64_t)res * res * res;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
  const int i[3] = {(int)(idx / ((int64_t)res * res)), (int)((idx / res) % res), (int)(idx % res)};
  int bc[3], l[3];
  float t[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    bc[d] = min(i[d] / bs, nb - 1);
    l[d] = i[d] - bc[d] * bs;
    const int len = min((bc[d] + 1) * bs, res - 1) - bc[d] * bs;
    t[d] = (float)l[d] / (float)len;
  }
  // the (up to eight) bricks that contain the sample
  const int ex = (l[0] == 0 && bc[0] > 0) ? 1 : 0, ey = (l[1] == 0 && bc[1] > 0) ? 1 : 0, ez = (l[2] == 0 && bc[2] > 0) ? 1 : 0;
  bool listed = false;
  for (int dx = 0; dx <= ex; ++dx)
    for (int dy = 0; dy <= ey; ++dy)
      for (int dz = 0; dz <= ez; ++dz)
        listed |= sg_state(state, ((bc[0] - dx) * nb + bc[1] - dy) * nb + bc[2] - dz) != 0;
  if (listed) continue;
  float c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = lat[((int64_t)(bc[0] + (k >> 2)) * nl + bc[1] + ((k >> 1) & 1)) * nl + bc[2] + (k & 1)];
  float mn = c[0], mx = c[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) { mn = fminf(mn, c[k]); mx = fmaxf(mx, c[k]); }
  auto mix = [](float a, float b, float w) { return (1.f - w) * a + w * b; };
  const float c00 = mix(c[0], c[4], t[0]), c01 = mix(c[1], c[5], t[0]), c10 = mix(c[2], c[6], t[0]), c11 = mix(c[3], c[7], t[0]);
  const float v = mix(mix(c00, c10, t[1]), mix(c01, c11, t[1]), t[2]);
  vol[idx] = fminf(fmaxf(v, mn), mx);
  }
}

int launch_sparse_classify(const SparseGeom& sg, const float* lattice, uint32_t* state, int32_t* list, int64_t* n_listed,
                           hipStream_t s) {
  const int64_t nbr = (int64_t)sg.nb * sg.nb * sg.nb;
  hipLaunchKernelGGL(sparse_classify_kernel, dim3(blocks_for(nbr, 256)), dim3(256), 0, s, sg, lattice, state, list,
                     reinterpret_cast<unsigned long long*>(n_listed));
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
int launch_sparse_grow(const SparseGeom& sg, const float* volume, int64_t first, int64_t count, uint32_t* state, int32_t* list,
                       int64_t* n_listed, hipStream_t s) {
  hipLaunchKernelGGL(sparse_grow_kernel, dim3((unsigned)count), dim3(256), 0, s, sg, volume, first, state, list,
                     reinterpret_cast<unsigned long long*>(n_listed));
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
int launch_sparse_fill(const SparseGeom& sg, const float* lattice, const uint32_t* state, float* volume, hipStream_t s) {
  const int64_t n = (int64_t)sg.res * sg.res * sg.res;
  const int64_t blocks = (n + 255) / 256;   // (a launch holds fewer than 2^32 threads: larger grids take several passes)
  hipLaunchKernelGGL(sparse_fill_kernel, dim3((unsigned)(blocks < (1 << 22) ? blocks : (1 << 22))), dim3(256), 0, s, sg, lattice,
                     state, volume);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

}  // namespace rnb
