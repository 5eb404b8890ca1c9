// Per-step ray / target generation of train_rnb on the device.
//
// The reference does this on the host every step: two CPU randint draws, CPU fancy-indexing of the
// [n_images, n_lights, H, W, 3] image / light tensors, three H2D copies and a D2H of the pixel indices
// (models/dataset.py:351-376, exp_runner.py:174-180, :214-220).  At ~10^5 rays/s that round trip is longer than
// the render step.  Here the image stack stays in HBM and one launch produces everything a step consumes.
#include "rnb_internal.h"

namespace rnb {

// The pixel-to-ray arithmetic, written once: the forward kernel and camera_adjoint_kernel both call it, so stack mode and
// source mode give the same bits and the adjoint differentiates exactly what the forward computed.
// p = Kinv[:3,:3] (x, y, 1) (dataset.py:365-367; same left-to-right accumulation as a 3-term dot product), nrm = ||p||,
// v = p / nrm, rays_v = d = R v, rays_o = o = t (dataset.py:369-373).  `kinv`, `pose`: row-major [4,4] (or their first 3 rows).
__device__ __forceinline__ void pixel_ray(const float* kinv, const float* pose, float fx, float fy, float& nrm, float v[3],
                                          float o[3], float d[3]) {
  float p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = kinv[r * 4 + 0] * fx + kinv[r * 4 + 1] * fy + kinv[r * 4 + 2] * 1.f;
  nrm = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  v[0] = p[0] / nrm; v[1] = p[1] / nrm; v[2] = p[2] / nrm;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    d[r] = pose[r * 4 + 0] * v[0] + pose[r * 4 + 1] * v[1] + pose[r * 4 + 2] * v[2];
    o[r] = pose[r * 4 + 3];
  }
}

// data row b = rays_o | rays_v | mask (dataset.py:376) and near / far of the unit sphere (dataset.py:448-458)
__device__ __forceinline__ void store_ray(float* data, float* near, float* far, int64_t b, const float o[3], const float d[3],
                                          float mask) {
  float* row = data + b * 7;
  row[0] = o[0]; row[1] = o[1]; row[2] = o[2];
  row[3] = d[0]; row[4] = d[1]; row[5] = d[2];
  row[6] = mask;
  if (near) {
    const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const float bq = 2.f * (o[0] * d[0] + o[1] * d[1] + o[2] * d[2]);
    const float mid = 0.5f * (-bq) / a;
    near[b] = mid - 1.f;
    far[b] = mid + 1.f;
  }
}

// nearest pixel, ties to even (torch.round); the clamp only guards the gathers against coordinates outside the image
__device__ __forceinline__ int64_t nearest_pixel(float fx, float fy, int H, int W) {
  const int64_t x = min(max((int64_t)rintf(fx), (int64_t)0), (int64_t)W - 1);
  const int64_t y = min(max((int64_t)rintf(fy), (int64_t)0), (int64_t)H - 1);
  return y * W + x;
}

// One launch makes rays [0, n) of one of two fronts with one of two target sources (four instantiations of raygen_kernel):
//   front    list: the integer pixels px[b], py[b] of a train step (dataset.py:351-376), gathers at y * W + x (the indices
//                  are range-checked in Python), all lights.
//            grid: rays [first, first + n) of the row-major Hl x Wl grid of a whole view (gen_rays_at / gen_rays_between,
//                  dataset.py:300-326, :401-446) at the float coordinates tx, ty, gathers at the rounded pixel
//                  (exp_runner.py:409-410: pixels.round().long()), all lights or the one light `light`.
//   targets  stack: mask, colours and lights gathered from the finished stacks of Dataset.__init__.
//            maps:  the same computed from the view's normal / albedo / mask maps (source mode, below).
struct RayArgs {           // (what every instantiation reads comes first: these small kernels wait on their argument loads)
  const float* kinv;       // [4,4] inverse intrinsics (row-major)
  const float* pose;       // [4,4] camera-to-world pose of the rays (grid: may be an interpolated one)
  const int64_t* px;       // list: [n]
  const int64_t* py;       // list: [n]
  int64_t n;               // rays of this launch
  int L, H, W, Cm;         // (maps: L, H, W are the source's, filled in by launch_rays)
  float* data;             // [n,7] = rays_o | rays_v | mask[..., :1]      (dataset.py:376)
  float* rgb;              // [Lo,n,3] or NULL (Lo = L, or 1 with light >= 0)
  float* rgb_wu;           // [Lo,n,3] or NULL
  float* lights_out;       // [Lo,n,3] or NULL
  float* near;             // [n] or NULL                                 (dataset.py:448-458)
  float* far;              // [n] or NULL
  rnb_source_maps_t src;   // maps (filled in by launch_rays)
  const float* view_pose;  // grid + maps: [4,4] pose of the view the maps belong to (rotates its lights to world space)
  const float* tx;         // grid: [Wl] pixel x of a grid column
  const float* ty;         // grid: [Hl] pixel y of a grid row
  int64_t first;           // grid
  int Wl;                  // grid
  int light;               // grid: one light, or -1 = all
  const float* images;     // stack: [L,H,W,3] or NULL
  const float* images_wu;  // stack: [L,H,W,3] or NULL
  const float* mask;       // stack: [H,W,Cm], or NULL (grid: the pose-only view, mask 0)
  const float* lights;     // stack: [L,H,W,3] or NULL
};

// the front: pixel coordinates of ray b and the pixel its targets come from
template <bool GRID>
__device__ __forceinline__ int64_t front_pixel(const RayArgs& g, int64_t b, float& fx, float& fy) {
  if constexpr (GRID) {
    const int64_t i = g.first + b;
    const int64_t iy = i / g.Wl;
    fx = g.tx[i - iy * g.Wl];
    fy = g.ty[iy];
    return nearest_pixel(fx, fy, g.H, g.W);
  } else {
    const int64_t x = g.px[b], y = g.py[b];
    fx = (float)x;
    fy = (float)y;
    return y * g.W + x;
  }
}

// stack targets: pixel `pix` of the lights [l0, l0 + Lo) gathered to row b of the [Lo, n, 3] outputs
__device__ __forceinline__ void stack_targets(const RayArgs& g, int64_t pix, int l0, int Lo, int64_t b) {
  const int64_t plane = (int64_t)g.H * g.W * 3;
  for (int lo = 0; lo < Lo; ++lo) {
    const int64_t src = (l0 + lo) * plane + pix * 3;
    const int64_t dst = ((int64_t)lo * g.n + b) * 3;
    if (g.rgb) { g.rgb[dst] = g.images[src]; g.rgb[dst + 1] = g.images[src + 1]; g.rgb[dst + 2] = g.images[src + 2]; }
    if (g.rgb_wu) {
      g.rgb_wu[dst] = g.images_wu[src]; g.rgb_wu[dst + 1] = g.images_wu[src + 1]; g.rgb_wu[dst + 2] = g.images_wu[src + 2];
    }
    if (g.lights_out) {
      g.lights_out[dst] = g.lights[src]; g.lights_out[dst + 1] = g.lights[src + 1]; g.lights_out[dst + 2] = g.lights[src + 2];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Source mode: the same outputs computed from a view's normal / albedo / mask maps instead of gathered from the finished
// stacks of Dataset.__init__ (models/dataset.py:100-298).  Everything in those stacks is a function of one pixel:
//   decode     c = v / M (M = 255 or 65535), normal n = 2c - 1 with y and z negated, albedo = c, mask = (c > 0.5)
//              (dataset.py:48-68, :134-136)
//   frame      gen_light_directions(normal) rotates the fixed lights u_k by a rotation R whose third column is
//              a = +-n/|n| with a_z >= 0; its first two columns are whatever basis LAPACK's SVD of n n^T returned for the
//              repeated zero singular value.  Here they are b1, b2 of Duff et al., "Building an Orthonormal Basis,
//              Revisited" (sign = +1, non-singular because a_z >= 0; b1 x b2 = a): a pure function of the normal.
//   lights     l_k = u_k.x b1 + u_k.y b2 + u_k.z a (camera space), lights_dir_k = view_pose[:3,:3] l_k
//   colours    albedo max(n . l_k, 0) and albedo max(n . w_k, 0) for the warm-up lights w_k, with the raw n (relu_nan: a
//              NaN stays NaN, as with np.maximum)
// IEEE sqrt and division throughout (this file is compiled without contraction).
__device__ __forceinline__ void load3(const void* base, int type, int64_t at, float c[3]) {
  if (type == RNB_SOURCE_U8) {
    const uint8_t* q = (const uint8_t*)base + at;
    c[0] = (float)q[0] / 255.f; c[1] = (float)q[1] / 255.f; c[2] = (float)q[2] / 255.f;
  } else if (type == RNB_SOURCE_U16) {
    const uint16_t* q = (const uint16_t*)base + at;
    c[0] = (float)q[0] / 65535.f; c[1] = (float)q[1] / 65535.f; c[2] = (float)q[2] / 65535.f;
  } else {
    const float* q = (const float*)base + at;
    c[0] = q[0]; c[1] = q[1]; c[2] = q[2];
  }
}

__device__ __forceinline__ float source_mask(const rnb_source_maps_t& s, int64_t pix) {
  const int64_t at = pix * s.mask_channels;
  float c;
  if (s.mask_type == RNB_SOURCE_U8) c = (float)((const uint8_t*)s.mask)[at] / 255.f;
  else if (s.mask_type == RNB_SOURCE_U16) c = (float)((const uint16_t*)s.mask)[at] / 65535.f;
  else c = ((const float*)s.mask)[at];
  return c > 0.5f ? 1.f : 0.f;
}

// Colours and lights of pixel `pix` for the lights [l0, l0 + Lo), written to row b of [Lo, stride, 3] outputs.
__device__ __forceinline__ void source_targets(const rnb_source_maps_t& s, const float* view_pose, int64_t pix, int l0, int Lo,
                                               int64_t stride, int64_t b, float* rgb, float* rgb_wu, float* lights_out) {
  float n[3], alb[3] = {1.f, 1.f, 1.f};
  if (s.normals_type == RNB_SOURCE_F32) {
    load3(s.normals, RNB_SOURCE_F32, pix * 3, n);
  } else {
    float c[3];
    load3(s.normals, s.normals_type, pix * 3, c);
    n[0] = 2.f * c[0] - 1.f; n[1] = -(2.f * c[1] - 1.f); n[2] = -(2.f * c[2] - 1.f);
  }
  if (s.albedo) load3(s.albedo, s.normals_type, pix * 3, alb);
  float a[3] = {0.f, 0.f, 1.f}, b1[3], b2[3];
  if (rgb || lights_out) {
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (len != 0.f) { a[0] = n[0] / len; a[1] = n[1] / len; a[2] = n[2] / len; }   // (a NaN normal stays NaN)
    if (a[2] < 0.f) { a[0] = -a[0]; a[1] = -a[1]; a[2] = -a[2]; }
    const float q = -1.f / (1.f + a[2]);
    const float r = a[0] * a[1] * q;
    b1[0] = 1.f + a[0] * a[0] * q; b1[1] = r; b1[2] = -a[0];
    b2[0] = r; b2[1] = 1.f + a[1] * a[1] * q; b2[2] = -a[1];
  }
  for (int lo = 0; lo < Lo; ++lo) {
    const int l = l0 + lo;
    const int64_t dst = ((int64_t)lo * stride + b) * 3;
    if (rgb || lights_out) {
      const float* u = s.local_lights[l];
      float lc[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) lc[k] = u[0] * b1[k] + u[1] * b2[k] + u[2] * a[k];
      if (rgb) {
        const float shade = relu_nan(n[0] * lc[0] + n[1] * lc[1] + n[2] * lc[2]);
        rgb[dst] = alb[0] * shade; rgb[dst + 1] = alb[1] * shade; rgb[dst + 2] = alb[2] * shade;
      }
      if (lights_out) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          lights_out[dst + k] = view_pose[k * 4 + 0] * lc[0] + view_pose[k * 4 + 1] * lc[1] + view_pose[k * 4 + 2] * lc[2];
      }
    }
    if (rgb_wu) {
      const float* w = s.warmup_lights_cam[l];
      const float shade = relu_nan(n[0] * w[0] + n[1] * w[1] + n[2] * w[2]);
      rgb_wu[dst] = alb[0] * shade; rgb_wu[dst + 1] = alb[1] * shade; rgb_wu[dst + 2] = alb[2] * shade;
    }
  }
}

template <bool GRID, bool MAPS>
__global__ void raygen_kernel(RayArgs g) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= g.n) return;
  float fx, fy, nrm, v[3], o[3], d[3];
  const int64_t pix = front_pixel<GRID>(g, b, fx, fy);
  pixel_ray(g.kinv, g.pose, fx, fy, nrm, v, o, d);
  const int l0 = GRID && g.light >= 0 ? g.light : 0;
  const int Lo = GRID && g.light >= 0 ? 1 : g.L;
  if constexpr (MAPS) {
    store_ray(g.data, g.near, g.far, b, o, d, source_mask(g.src, pix));
    if (g.rgb || g.rgb_wu || g.lights_out)
      source_targets(g.src, GRID ? g.view_pose : g.pose, pix, l0, Lo, g.n, b, g.rgb, g.rgb_wu, g.lights_out);
  } else {
    store_ray(g.data, g.near, g.far, b, o, d, g.mask ? g.mask[pix * g.Cm] : 0.f);
    stack_targets(g, pix, l0, Lo, b);
  }
}

// the source maps' own checks (check_rays)
static int check_source_maps(const char* who, const rnb_source_maps_t* src) {
  if (!src) RNB_FAIL(RNB_E_NULL, "%s: NULL source maps", who);
  if (!src->normals || !src->mask) RNB_FAIL(RNB_E_NULL, "%s: NULL normals or mask", who);
  if (src->normals_type < RNB_SOURCE_U8 || src->normals_type > RNB_SOURCE_F32 || src->mask_type < RNB_SOURCE_U8 ||
      src->mask_type > RNB_SOURCE_F32)
    RNB_FAIL(RNB_E_INVALID, "%s: unknown element type code (normals / albedo %d, mask %d)", who, src->normals_type,
             src->mask_type);
  if (src->n_lights < 1 || src->n_lights > kMaxRenderLights)
    RNB_FAIL(RNB_E_INVALID, "%s: n_lights %d outside 1..kMaxRenderLights (%d)", who, src->n_lights, kMaxRenderLights);
  if (src->H < 1 || src->W < 1 || src->mask_channels < 1)
    RNB_FAIL(RNB_E_INVALID, "%s: bad shape (H %d, W %d, mask channels %d)", who, src->H, src->W, src->mask_channels);
  return RNB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Camera adjoint: d loss / d pose and d loss / d intrinsics_inv from the adjoints of what pixel_ray + store_ray (and,
// in source mode, the light rotation of source_targets) made of them.  Per ray, recomputed from its pixel:
//   p = Kinv[:3,:3] (x, y, 1), n = |p|, v = p / n, d = R v, o = t, a = d.d, mid = -(o.d) / a, near / far = mid -+ 1
//   m_bar = near_bar + far_bar;  o_bar += -m_bar d / a;  d_bar += -m_bar o / a + 2 m_bar (o.d) d / a^2
//   pose_bar[:3,3] = sum_b o_bar;  pose_bar[:3,:3] = sum_b d_bar v^T + sum_{l,b} l_bar (R^T l)^T   (lights = R l_cam)
//   v_bar = R^T d_bar;  p_bar = (v_bar - v (v.v_bar)) / n;  intrinsics_inv_bar[:3,:3] = sum_b p_bar (x, y, 1)^T
// One workgroup: every lane sums its rays b = lane, lane + 256, ... in that order (the ray's own terms, then its lights
// in light order), a shuffle butterfly per wave, the four waves combined through LDS in wave order.  No atomics: the
// bits depend on the inputs only.
constexpr int kCamAdjThreads = 256;
constexpr int kCamAdjTerms = 21;   // pose_bar[:3,:3] (9) | pose_bar[:3,3] (3) | intrinsics_inv_bar[:3,:3] (9)

struct CameraAdjArgs {
  const float* kinv;        // [4,4]
  const float* pose;        // [4,4]
  const int64_t* px;        // [B]
  const int64_t* py;        // [B]
  int64_t B;
  const float* lights;      // [L,B,3] the forward's lights_dir, or NULL
  int L;
  const float* o_bar;       // [B,3] or NULL
  const float* d_bar;       // [B,3] or NULL
  const float* lights_bar;  // [L,B,3] or NULL
  const float* near_bar;    // [B] or NULL
  const float* far_bar;     // [B] or NULL
  float* pose_bar;          // [4,4]
  float* kinv_bar;          // [4,4] or NULL
};

__device__ __forceinline__ float cam_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kCamAdjThreads) void camera_adjoint_kernel(CameraAdjArgs g) {
  __shared__ float red[kCamAdjThreads / 64][kCamAdjTerms];
  float acc[kCamAdjTerms];
#pragma unroll
  for (int k = 0; k < kCamAdjTerms; ++k) acc[k] = 0.f;
  float P[3][4];   // the pose's rotation | translation
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) P[r][c] = g.pose[r * 4 + c];
  const bool with_lights = g.lights != nullptr && g.lights_bar != nullptr;
  for (int64_t b = threadIdx.x; b < g.B; b += kCamAdjThreads) {
    const float q[3] = {(float)g.px[b], (float)g.py[b], 1.f};
    float nrm, v[3], o[3], d[3];
    pixel_ray(g.kinv, &P[0][0], q[0], q[1], nrm, v, o, d);
    float ob[3] = {0.f, 0.f, 0.f}, db[3] = {0.f, 0.f, 0.f};
    if (g.o_bar)
      for (int r = 0; r < 3; ++r) ob[r] = g.o_bar[b * 3 + r];
    if (g.d_bar)
      for (int r = 0; r < 3; ++r) db[r] = g.d_bar[b * 3 + r];
    const float mb = (g.near_bar ? g.near_bar[b] : 0.f) + (g.far_bar ? g.far_bar[b] : 0.f);
    if (g.near_bar || g.far_bar) {
      const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      const float od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2];
      const float s = mb / a;
      const float t = 2.f * s * od / a;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        ob[r] -= s * d[r];
        db[r] += t * d[r] - s * o[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[r * 3 + c] += db[r] * v[c];
      acc[9 + r] += ob[r];
    }
    if (g.kinv_bar) {
      float vb[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) vb[c] = P[0][c] * db[0] + P[1][c] * db[1] + P[2][c] * db[2];
      const float vv = v[0] * vb[0] + v[1] * vb[1] + v[2] * vb[2];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float pb = (vb[r] - v[r] * vv) / nrm;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[12 + r * 3 + c] += pb * q[c];
      }
    }
    if (with_lights) {
      for (int l = 0; l < g.L; ++l) {
        const int64_t at = ((int64_t)l * g.B + b) * 3;
        const float lw[3] = {g.lights[at], g.lights[at + 1], g.lights[at + 2]};
        const float lb[3] = {g.lights_bar[at], g.lights_bar[at + 1], g.lights_bar[at + 2]};
        float lc[3];   // R^T l: the camera-space light the forward rotated
#pragma unroll
        for (int c = 0; c < 3; ++c) lc[c] = P[0][c] * lw[0] + P[1][c] * lw[1] + P[2][c] * lw[2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[r * 3 + c] += lb[r] * lc[c];
      }
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kCamAdjTerms; ++k) {
    const float s = cam_wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[wave][k] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < kCamAdjTerms) {
    const float s = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    if (k < 9) g.pose_bar[(k / 3) * 4 + k % 3] = s;
    else if (k < 12) g.pose_bar[(k - 9) * 4 + 3] = s;
    else if (g.kinv_bar) g.kinv_bar[((k - 12) / 3) * 4 + (k - 12) % 3] = s;
  } else if (k < kCamAdjTerms + 4) {
    g.pose_bar[12 + (k - kCamAdjTerms)] = 0.f;                      // the pose's last row
  } else if (k < kCamAdjTerms + 11 && g.kinv_bar) {
    const int z = k - (kCamAdjTerms + 4);                           // intrinsics_inv's last column (3) and last row (4)
    g.kinv_bar[z < 3 ? z * 4 + 3 : 12 + (z - 3)] = 0.f;
  }
}

}  // namespace rnb

#define RNB_API extern "C" __attribute__((visibility("default")))

RNB_API int rnb_gen_rays_camera_bwd(const float* intrinsics_inv, const float* pose, const int64_t* pixels_x,
                                    const int64_t* pixels_y, int64_t B, const float* lights_dir, int32_t n_lights,
                                    const float* rays_o_bar, const float* rays_d_bar, const float* lights_bar,
                                    const float* near_bar, const float* far_bar, float* pose_bar, float* intrinsics_inv_bar,
                                    rnb_stream_t stream) {
  using namespace rnb;
  if (!intrinsics_inv || !pose || !pixels_x || !pixels_y || !pose_bar)
    RNB_FAIL(RNB_E_NULL, "rnb_gen_rays_camera_bwd: NULL pointer");
  if (lights_bar && !lights_dir) RNB_FAIL(RNB_E_NULL, "rnb_gen_rays_camera_bwd: lights_bar without the forward's lights_dir");
  if (B < 1) RNB_FAIL(RNB_E_INVALID, "rnb_gen_rays_camera_bwd: bad shape (B %lld)", (long long)B);
  if (n_lights < 0 || n_lights > kMaxRenderLights || (lights_dir && n_lights < 1))
    RNB_FAIL(RNB_E_INVALID, "rnb_gen_rays_camera_bwd: n_lights %d outside %d..kMaxRenderLights (%d)", n_lights,
             lights_dir ? 1 : 0, kMaxRenderLights);
  CameraAdjArgs g{intrinsics_inv, pose, pixels_x, pixels_y, B, lights_dir, n_lights, rays_o_bar, rays_d_bar, lights_bar,
                  near_bar, far_bar, pose_bar, intrinsics_inv_bar};
  hipLaunchKernelGGL(camera_adjoint_kernel, dim3(1), dim3(kCamAdjThreads), 0, (hipStream_t)stream, g);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

// What the four forward entry points refuse (each message prefixed by the entry point's name), all before any launch.
template <bool GRID, bool MAPS>
static int check_rays(const char* who, const rnb::RayArgs& g, const rnb_source_maps_t* source, int Hl) {
  using namespace rnb;
  if (!g.kinv || !g.pose || !g.data || (GRID ? !g.tx || !g.ty : !g.px || !g.py) || (GRID && MAPS && !g.view_pose) ||
      (!GRID && !MAPS && !g.mask))
    RNB_FAIL(RNB_E_NULL, "%s: NULL pointer", who);
  if (MAPS) RNB_TRY(check_source_maps(who, source));
  else if ((g.rgb && !g.images) || (g.rgb_wu && !g.images_wu) || (g.lights_out && !g.lights))
    RNB_FAIL(RNB_E_NULL, "%s: output requested without its source", who);
  if ((g.near == nullptr) != (g.far == nullptr)) RNB_FAIL(RNB_E_NULL, "%s: near and far come together", who);
  if (!MAPS && (g.L < 0 || g.H < 1 || g.W < 1 || (g.mask && g.Cm < 1)))
    RNB_FAIL(RNB_E_INVALID, "%s: bad shape (L %d, H %d, W %d, mask channels %d)", who, g.L, g.H, g.W, g.Cm);
  if (!GRID) {
    if (g.n < 1) RNB_FAIL(RNB_E_INVALID, "%s: bad shape (B %lld)", who, (long long)g.n);
    return RNB_OK;
  }
  if (g.Wl < 1 || Hl < 1) RNB_FAIL(RNB_E_INVALID, "%s: bad shape (grid %d x %d)", who, Hl, g.Wl);
  if (g.first < 0 || g.n < 1 || g.first + g.n > (int64_t)Hl * g.Wl)
    RNB_FAIL(RNB_E_INVALID, "%s: rays [%lld, %lld) outside the %d x %d grid", who, (long long)g.first,
             (long long)(g.first + g.n), Hl, g.Wl);
  const int L = MAPS ? source->n_lights : g.L;
  if (g.light < -1 || g.light >= L)
    RNB_FAIL(RNB_E_INVALID, "%s: light %d out of range (n_lights %d; -1 = all)", who, g.light, L);
  return RNB_OK;
}

// The one launch path: the checks, then raygen_kernel<GRID, MAPS> over g.n rays.
template <bool GRID, bool MAPS>
static int launch_rays(const char* who, rnb::RayArgs g, const rnb_source_maps_t* source, int Hl, rnb_stream_t stream) {
  using namespace rnb;
  RNB_TRY((check_rays<GRID, MAPS>(who, g, source, Hl)));
  if (MAPS) {
    g.src = *source;
    g.L = source->n_lights; g.H = source->H; g.W = source->W;
  }
  hipLaunchKernelGGL((raygen_kernel<GRID, MAPS>), dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
  RNB_CHECK_LAUNCH();
  return RNB_OK;
}

RNB_API int rnb_gen_rays_at_view(const float* intrinsics_inv, const float* pose, const float* images,
                                 const float* images_warmup, const float* mask, int32_t mask_channels,
                                 const float* light_directions, const int64_t* pixels_x, const int64_t* pixels_y,
                                 int64_t B, int32_t n_lights, int32_t H, int32_t W, float* data, float* true_rgb,
                                 float* true_rgb_warmup, float* lights_dir, float* near, float* far,
                                 rnb_stream_t stream) {
  rnb::RayArgs g{intrinsics_inv, pose, pixels_x, pixels_y, B, n_lights, H, W, mask_channels, data, true_rgb, true_rgb_warmup,
                 lights_dir, near, far, {}, nullptr, nullptr, nullptr, 0, 0, -1, images, images_warmup, mask, light_directions};
  return launch_rays<false, false>("rnb_gen_rays_at_view", g, nullptr, 0, stream);
}

RNB_API int rnb_gen_rays_grid(const float* intrinsics_inv, const float* pose, const float* tx, const float* ty, int32_t Wl,
                              int32_t Hl, int64_t first, int64_t n, const float* images, const float* images_warmup,
                              const float* mask, int32_t mask_channels, const float* light_directions,
                              int32_t n_lights, int32_t light, int32_t H, int32_t W, float* data, float* true_rgb,
                              float* true_rgb_warmup, float* lights_dir, float* near, float* far, rnb_stream_t stream) {
  rnb::RayArgs g{intrinsics_inv, pose, nullptr, nullptr, n, n_lights, H, W, mask_channels, data, true_rgb, true_rgb_warmup,
                 lights_dir, near, far, {}, nullptr, tx, ty, first, Wl, light, images, images_warmup, mask, light_directions};
  return launch_rays<true, false>("rnb_gen_rays_grid", g, nullptr, Hl, stream);
}

RNB_API int rnb_gen_rays_at_view_from_maps(const float* intrinsics_inv, const float* pose, const rnb_source_maps_t* source,
                                           const int64_t* pixels_x, const int64_t* pixels_y, int64_t B, float* data,
                                           float* true_rgb, float* true_rgb_warmup, float* lights_dir, float* near, float* far,
                                           rnb_stream_t stream) {
  rnb::RayArgs g{intrinsics_inv, pose, pixels_x, pixels_y, B, 0, 0, 0, 0, data, true_rgb, true_rgb_warmup, lights_dir, near, far,
                 {}, nullptr, nullptr, nullptr, 0, 0, -1, nullptr, nullptr, nullptr, nullptr};
  return launch_rays<false, true>("rnb_gen_rays_at_view_from_maps", g, source, 0, stream);
}

RNB_API int rnb_gen_rays_grid_from_maps(const float* intrinsics_inv, const float* pose, const float* view_pose,
                                        const float* tx, const float* ty, int32_t Wl, int32_t Hl, int64_t first, int64_t n,
                                        const rnb_source_maps_t* source, int32_t light, float* data, float* true_rgb,
                                        float* true_rgb_warmup, float* lights_dir, float* near, float* far,
                                        rnb_stream_t stream) {
  rnb::RayArgs g{intrinsics_inv, pose, nullptr, nullptr, n, 0, 0, 0, 0, data, true_rgb, true_rgb_warmup, lights_dir, near, far,
                 {}, view_pose, tx, ty, first, Wl, light, nullptr, nullptr, nullptr, nullptr};
  return launch_rays<true, true>("rnb_gen_rays_grid_from_maps", g, source, Hl, stream);
}
