// Texture baking on the device: the per-triangle atlas of a (simplified) mesh, its lattice samples and the two 8-bit images
// (rnb_texture_sample_points, rnb_texture_pack in include/rnbneus.h; DESIGN.md "Texture baking").
//
//   samples  tb_sample_kernel   one lane per sample p = t n_s + r: r -> (a1, a2), the three weights, the point in fp64 -> fp32
//   images   tb_pack_kernel     one lane per texel: cell -> half -> triangle, (a1, a2) -> sample index, one 4-byte store per image
//
// Pure integer arithmetic decides which triangle and which sample a texel shows; the field is evaluated between the two
// kernels by rnb_mesh_vertex_attrs on the sample points.  No atomics except the bad-triangle counter (one integer add per
// wave).  The file is compiled with -ffp-contract=off: the sample point is (w0 A + w1 B) + w2 C with every product and sum
// rounded on its own, which is what makes the samples of a shared edge equal from both sides (tests/texture_bake_ref.py is
// the same expression in numpy).
//
// WHY NOTHING RUNS AWAY.  The only loop is the search of the row a2 of a rank r, s + 1 <= 256 trips fixed before it starts
// (no break).  Every address is an index checked against its array: vertex indices against V before the vertices are read
// (mesh_corners of mesh_common.hip.h), the sample index against T n_s before rgb / normal are read, the texel and the
// sample against the launch sizes.
#include "mesh_common.hip.h"

namespace rnb {

constexpr int kTbThreads = 256;

struct TbMesh {
  const double* vertices;
  int64_t V;
  const int32_t* tri;
  int64_t T;
};

// r(a1, a2) = a2 (s + 1) - a2 (a2 - 1) / 2 + a1: rows of constant a2, row a2 holds s + 1 - a2 samples
__device__ inline int tb_rank(int s, int a1, int a2) { return a2 * (s + 1) - a2 * (a2 - 1) / 2 + a1; }

// one add of the number of lanes with `pred` per wave
__device__ inline void tb_wave_count(long long* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
    atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kTbThreads) void tb_sample_kernel(TbMesh m, int s, int n_s, int64_t first, int64_t count,
                                                               float* __restrict__ points, long long* bad_out) {
  const int64_t i = (int64_t)blockIdx.x * kTbThreads + threadIdx.x;
  const bool live = i < count;
  bool bad_first = false;
  float out[3] = {0.0f, 0.0f, 0.0f};
  if (live) {
    const unsigned p = (unsigned)(first + i);              // < T n_s < 2^31 (checked by the host)
    const int64_t t = (int64_t)(p / (unsigned)n_s);
    const int r = (int)(p % (unsigned)n_s);
    int a2 = 0;
    for (int row = 0; row <= s; ++row)                     // the last row whose first rank is <= r
      a2 = tb_rank(s, 0, row) <= r ? row : a2;
    const int a1 = r - tb_rank(s, 0, a2);
    double c[9];
    if (t < m.T && mesh_corners(m.vertices, m.V, m.tri, t, c)) {
      const double sd = (double)s;
      const double w0 = (double)(s - a1 - a2) / sd, w1 = (double)a1 / sd, w2 = (double)a2 / sd;
#pragma unroll
      for (int d = 0; d < 3; ++d) out[d] = (float)((w0 * c[d] + w1 * c[3 + d]) + w2 * c[6 + d]);
    } else {
      bad_first = r == 0;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) points[i * 3 + d] = out[d];
  }
  if (bad_out) tb_wave_count(bad_out, bad_first);
}

struct TbPack {
  TbMesh m;
  int s, c, cols, W, H, n_s;
  int64_t N;                       // T n_s: the rows of rgb / normal
  const uint8_t* rgb;
  const float* normal;
  uint32_t* albedo_image;
  uint32_t* normal_image;
  int32_t* texel_sample;
};

__device__ inline unsigned tb_quantize(float n) {
  const float v = (0.5f * n + 0.5f) * 255.0f;
  return v >= 0.0f ? (v <= 255.0f ? (unsigned)rintf(v) : 255u) : 0u;   // NaN: 0
}

__global__ __launch_bounds__(kTbThreads) void tb_pack_kernel(TbPack a) {
  const int64_t texel = (int64_t)blockIdx.x * kTbThreads + threadIdx.x;
  if (texel >= (int64_t)a.W * a.H) return;
  const int x = (int)(texel % a.W), y = (int)(texel / a.W);
  const int cx = x / a.c, cy = y / a.c;
  int64_t smp = -1;
  if (cx < a.cols) {
    const int i = x - cx * a.c, j = y - cy * a.c;
    const bool up = i + j > a.s + 3;
    const int64_t t = 2 * ((int64_t)cy * a.cols + cx) + (up ? 1 : 0);
    if (t < a.m.T) {
      int a1 = up ? a.c - 2 - i : i - 1;
      a1 = a1 < 0 ? 0 : (a1 > a.s ? a.s : a1);
      int a2 = up ? a.c - 2 - j : j - 1;
      a2 = a2 < 0 ? 0 : a2;
      a2 = a2 > a.s - a1 ? a.s - a1 : a2;
      double p[9];
      if (mesh_corners(a.m.vertices, a.m.V, a.m.tri, t, p)) smp = t * a.n_s + tb_rank(a.s, a1, a2);
    }
  }
  if (smp >= a.N) smp = -1;        // (cannot happen: t < T and r < n_s; an address is checked all the same)
  if (a.texel_sample) a.texel_sample[texel] = (int32_t)smp;
  if (a.albedo_image) {
    unsigned v = 0u;
    if (smp >= 0) v = (unsigned)a.rgb[smp * 3] | ((unsigned)a.rgb[smp * 3 + 1] << 8) | ((unsigned)a.rgb[smp * 3 + 2] << 16) | 0xff000000u;
    a.albedo_image[texel] = v;     // bytes r, g, b, a in memory order (little endian)
  }
  if (a.normal_image) {
    unsigned v = 0u;
    if (smp >= 0)
      v = tb_quantize(a.normal[smp * 3]) | (tb_quantize(a.normal[smp * 3 + 1]) << 8) | (tb_quantize(a.normal[smp * 3 + 2]) << 16) | 0xff000000u;
    a.normal_image[texel] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------

static unsigned tb_grid(int64_t n) { return (unsigned)((n + kTbThreads - 1) / kTbThreads); }

// V, T, s checked; *n_s and *N = T n_s < 2^31
static int tb_sizes(const char* who, int64_t V, int64_t T, int32_t s, int* n_s, int64_t* N) {
  RNB_TRY(mesh_sizes(who, V, T));
  if (s < 1 || s > 255) RNB_FAIL(RNB_E_INVALID, "%s: chart size s = %d outside [1, 255]", who, s);
  *n_s = (s + 1) * (s + 2) / 2;
  *N = T * (int64_t)*n_s;
  if (*N > kMeshMax) RNB_FAIL(RNB_E_INVALID, "%s: %lld triangles x %d samples is not below 2^31", who, (long long)T, *n_s);
  return RNB_OK;
}

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_texture_sample_points(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                      int32_t s, int64_t first, int64_t count, float* points_out, int64_t* bad_out,
                                      rnb_stream_t stream) {
  using namespace rnb;
  const int64_t V = n_vertices, T = n_triangles;
  int n_s;
  int64_t N;
  RNB_TRY(tb_sizes("rnb_texture_sample_points", V, T, s, &n_s, &N));
  if (first < 0 || count < 0 || first > N || count > N - first)
    RNB_FAIL(RNB_E_INVALID, "rnb_texture_sample_points: samples [%lld, %lld + %lld) outside [0, %lld)", (long long)first,
             (long long)first, (long long)count, (long long)N);
  if (!points_out) RNB_FAIL(RNB_E_INVALID, "rnb_texture_sample_points: every output is NULL");
  if (T == 0 || count == 0) return RNB_OK;
  if (!triangles || (V > 0 && !vertices)) RNB_FAIL(RNB_E_NULL, "rnb_texture_sample_points: NULL vertices / triangles");
  const TbMesh m{vertices, V, triangles, T};
  hipLaunchKernelGGL(tb_sample_kernel, dim3(tb_grid(count)), dim3(kTbThreads), 0, (hipStream_t)stream, m, (int)s, n_s, first,
                     count, points_out, (long long*)bad_out);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_texture_pack(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                             const rnb_texture_layout* layout, const uint8_t* rgb, const float* normal, uint8_t* albedo_image,
                             uint8_t* normal_image, int32_t* texel_sample, rnb_stream_t stream) {
  using namespace rnb;
  const int64_t V = n_vertices, T = n_triangles;
  if (!layout) RNB_FAIL(RNB_E_NULL, "rnb_texture_pack: NULL layout");
  int n_s;
  int64_t N;
  RNB_TRY(tb_sizes("rnb_texture_pack", V, T, layout->s, &n_s, &N));
  const int64_t c = layout->s + 5, cols = layout->cols, W = layout->W, H = layout->H, K = (T + 1) / 2;
  if (W < 0 || H < 0 || cols < 0 || W * H > kMeshMax)
    RNB_FAIL(RNB_E_INVALID, "rnb_texture_pack: layout %lld x %lld with %lld columns of cells: negative, or 2^31 texels or more",
             (long long)W, (long long)H, (long long)cols);
  if (cols * c > W || cols * (H / c) < K)
    RNB_FAIL(RNB_E_INVALID, "rnb_texture_pack: %lld columns of %lld-texel cells in %lld x %lld texels do not hold %lld triangles",
             (long long)cols, (long long)c, (long long)W, (long long)H, (long long)T);
  if (!albedo_image && !normal_image && !texel_sample) RNB_FAIL(RNB_E_INVALID, "rnb_texture_pack: every output is NULL");
  if (W * H == 0) return RNB_OK;
  hipStream_t st = (hipStream_t)stream;
  if (T == 0) {                    // every texel is empty: no kernel
    if (albedo_image) RNB_CHECK_HIP(hipMemsetAsync(albedo_image, 0, (size_t)(W * H) * 4, st));
    if (normal_image) RNB_CHECK_HIP(hipMemsetAsync(normal_image, 0, (size_t)(W * H) * 4, st));
    if (texel_sample) RNB_CHECK_HIP(hipMemsetAsync(texel_sample, 0xff, (size_t)(W * H) * 4, st));
    return RNB_OK;
  }
  if (!triangles || (V > 0 && !vertices)) RNB_FAIL(RNB_E_NULL, "rnb_texture_pack: NULL vertices / triangles");
  if ((albedo_image && !rgb) || (normal_image && !normal))
    RNB_FAIL(RNB_E_NULL, "rnb_texture_pack: an image without its samples (albedo_image needs rgb, normal_image needs normal)");
  const TbPack a{{vertices, V, triangles, T}, (int)layout->s, (int)c, (int)cols, (int)W, (int)H, n_s, N, rgb, normal,
                 (uint32_t*)albedo_image, (uint32_t*)normal_image, texel_sample};
  hipLaunchKernelGGL(tb_pack_kernel, dim3(tb_grid(W * H)), dim3(kTbThreads), 0, st, a);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}
