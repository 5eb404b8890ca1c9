/*
 * rnbneus.h — C ABI of librnbneus_hip.so, the MI355X (gfx950) implementation of the RNb-NeuS
 * volumetric SDF renderer hot path.
 *
 * The reference (rti-team-imvia/RNb-NeuS-fork) has no FFI layer: its boundary is the Python object
 * protocol between exp_runner.py and models/{embedder,fields,renderer}.py.  Each entry point below
 * names the reference interface it replaces (file:line relative to the reference root).  The Python
 * drop-in classes in rnb-neus-fork_amd/ bind these symbols with ctypes (INTEGRATION.md shows the
 * stub); nothing in the signatures depends on PyTorch: plain device pointers, sizes, a hipStream_t.
 *
 * Conventions
 *   - every function returns 0 on success or a negative RNB_E_* code; it never throws, never calls
 *     exit and never synchronises the device.  rnb_last_error_string() describes the last failure on
 *     the calling thread.
 *   - all pointers are DEVICE pointers to fp32 (or int32 where stated) unless marked host.
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library allocates nothing that
 *     outlives a call and keeps no mutable global state.  Work is enqueued on the given stream only.
 *   - tensors are dense row-major with the shapes given in brackets.
 */
#ifndef RNBNEUS_H
#define RNBNEUS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_ABI_VERSION 5
#define RNB_MAX_LIN 16 /* linear layers per MLP */

enum {
  RNB_OK = 0,
  RNB_E_INVALID = -1,     /* bad argument / unsupported configuration */
  RNB_E_WORKSPACE = -2,   /* workspace too small */
  RNB_E_HIP = -3,         /* a HIP runtime call or launch failed */
  RNB_E_NULL = -4         /* required pointer is NULL */
};

typedef void* rnb_stream_t; /* hipStream_t */

/* Constructor arguments of the three networks and the renderer, i.e. the `model { ... }` block of
 * confs/wmask_rnb.conf:53-90 as splatted into SDFNetwork(**conf) (models/fields.py:9-20),
 * RenderingNetwork(**conf) (models/fields.py:132-141) and NeuSRenderer(**conf)
 * (models/renderer.py:73-82). */
typedef struct rnb_model_desc {
  /* SDFNetwork */
  int32_t sdf_d_in;       /* must be 3 */
  int32_t sdf_d_out;      /* 1 + feature width (257) */
  int32_t sdf_d_hidden;   /* 256 */
  int32_t sdf_n_layers;   /* 8 hidden layers => 9 linear layers */
  int32_t sdf_skip_in;    /* single skip layer index (4) or -1 */
  int32_t sdf_multires;   /* 6 */
  float   sdf_scale;      /* 1.0 */
  int32_t sdf_weight_norm;
  /* RenderingNetwork, mode "no_view_dir" only */
  int32_t col_d_feature;  /* 256 */
  int32_t col_d_in;       /* 6 (points + normals; view dirs are ignored in this mode) */
  int32_t col_d_out;      /* 3 */
  int32_t col_d_hidden;   /* 256 */
  int32_t col_n_layers;   /* 2 hidden layers => 3 linear layers */
  int32_t col_multires_view; /* 4 */
  int32_t col_squeeze_out;   /* 1: sigmoid on the output */
  int32_t col_weight_norm;
  /* NeuSRenderer */
  int32_t n_samples;      /* 64 */
  int32_t n_importance;   /* 64 */
  int32_t up_sample_steps;/* 4 */
  int32_t variant;        /* RNB_VARIANT_* bits: arithmetic / kernel variant of this model instance (0 = default) */
} rnb_model_desc;

/* rnb_model_desc.variant.  Every switch is an explicit field of the descriptor that accompanies each call: the
 * library reads no environment variables and keeps no process-global tuning state.
 *   RNB_VARIANT_BF16          BASELINE config 5: the SDF-network sweeps (forward, reverse normal, their adjoints and
 *                             the weight gradients) take bf16 operands on v_mfma_f32_32x32x16_bf16 with fp32
 *                             accumulators; the per-point saved state is bf16.  Master weights, gradients, sampling,
 *                             the albedo network and the composite stay fp32.  Needs the 256-wide network shape.
 *   RNB_VARIANT_DETERMINISTIC split-K partial sums go to workspace slabs and are reduced in a fixed order instead of
 *                             through fp32 atomics: gradients are bit-reproducible from run to run and across ranks.
 *   RNB_VARIANT_GENERIC       per-layer GEMM chain for every sweep even when the fused kernels support the shape.
 *   RNB_VARIANT_DW_LDS        register-staged LDS weight-gradient GEMMs (the guarded generic kernel) for every job.
 *   RNB_VARIANT_DW_STAGED     256 x 256 weight gradients through the LDS-DMA staged kernel (one 16-wave workgroup owns a
 *                             whole gradient of a point range: every operand byte is fetched once, partial gradients
 *                             leave through slabs + an ordered reduction, no atomics) instead of the register-direct
 *                             128 x 128-tile kernel.  Halves the operand traffic of that launch; measured 2 % slower
 *                             per step, hence not the default.
 *   RNB_VARIANT_X3            fp32 products of the fused sweeps and of the 256 x 256 weight gradients on the bf16 matrix
 *                             pipe: each fp32 operand as three bf16 terms (hi + mid + lo = x exactly), six of the nine
 *                             cross terms per product, fp32 accumulate.  Same fp32 state, same results to fp32 rounding
 *                             (the dropped terms are < 2^-26 relative); rnb_packed_floats grows by the split weight
 *                             mirror (1.5 x).  This is what variant 0 selects for the 256-wide network shape; the bit
 *                             only makes the request explicit (an unsupported shape is then an error).
 *   RNB_VARIANT_F32_MFMA      the same kernels on v_mfma_f32_32x32x2_f32 (the round-1 arithmetic; A/B switch).
 *   RNB_VARIANT_*_TI/_NW      tile height (1: 32 points, 2: 64 points) / waves per workgroup (4 or 8) of the fused
 *                             backward sweeps (BWD) and of the fused forward (FWD); 0 = the measured default.
 *   RNB_VARIANT_REG_TILE /    which family of fused x3 sweeps runs: REG_TILE = the M/V kernels (sweep_mv.hip: matrix waves
 *   RNB_VARIANT_LDS_TILE      with 32 points each and the weights through an LDS-DMA ring + vector waves for the
 *                             epilogues), LDS_TILE = the 64-point LDS-tile kernels (fused.hip / fused_bwd.hip).  Neither
 *                             bit: the measured default per sweep and batch size.  A/B switches.
 *   RNB_VARIANT_X2H /         (with X3; ON by default, NO_X2H switches it off) every fp32 product of the fused path except the
 *   RNB_VARIANT_NO_X2H        RA sweep's is taken as THREE fp16 matrix terms (x = hi + lo in fp16 after a power-of-two scale)
 *                             instead of six bf16 ones: half the matrix time; operands represented to 2^-22 (rms 2^-23.6;
 *                             the measured SDF error against fp64 is below the six-term scheme's).  Every scale
 *                             is TAKEN FROM THE DATA, so there is no operand range [round 5; through ABI 4 weights beyond 255
 *                             and activations beyond 1023 gave inf / NaN]: the weights' per matrix (2^8 while max |w| < 64,
 *                             else the power of two that puts the maximum in [2^13, 2^14); table behind the mirror in the
 *                             packed buffer); activations', network inputs' and Jacobian rows' per 64-point tile and layer (2^6
 *                             while the tile stays below 256); the saved state's that the weight gradients read per launch
 *                             (from maxima the forward leaves in the workspace); loss adjoints' per tile / per launch from
 *                             their recorded maxima, so any loss scale works (a loss times 2^k gives gradients times 2^k bit
 *                             for bit, tested at k = +-40).  In the old range the SDF network's sweeps give the same bits as ABI 4's.  The RA
 *                             sweep is bound by its saved-state traffic and keeps the six bf16 terms.
 *   RNB_VARIANT_NO_DEAD_TILES the fused albedo backward (the default fp32 route) skips every 64-point tile whose colour adjoint
 *                             is exactly zero — the rays outside the mask — and FB and the weight-gradient jobs skip those
 *                             tiles with it: same outputs and gradients (a tile is skipped only where the full path would
 *                             have produced exact zeros, NaN semantics included).  This bit forces the full path
 *                             on every tile.  A/B switch; no effect on the other routes. */
enum {
  RNB_VARIANT_BF16 = 1,
  RNB_VARIANT_DETERMINISTIC = 2,
  RNB_VARIANT_GENERIC = 4,
  RNB_VARIANT_DW_LDS = 8,
  RNB_VARIANT_DW_STAGED = 16,
  RNB_VARIANT_X3 = 32,
  RNB_VARIANT_F32_MFMA = 64,
  RNB_VARIANT_BWD_TI_SHIFT = 8,   /* 2 bits: 0 default, 1, 2 */
  RNB_VARIANT_BWD_NW_SHIFT = 10,  /* 2 bits: 0 default, 1 = 4 waves, 2 = 8 waves */
  RNB_VARIANT_FWD_TI_SHIFT = 12,
  RNB_VARIANT_FWD_NW_SHIFT = 14,
  RNB_VARIANT_REG_TILE = 1 << 16,
  RNB_VARIANT_LDS_TILE = 1 << 17,
  RNB_VARIANT_X2H = 1 << 18,
  RNB_VARIANT_NO_X2H = 1 << 19,
  RNB_VARIANT_NO_DEAD_TILES = 1 << 20
};

/* Trainable leaves of one MLP in the reference's state_dict naming (linN.weight_g [out,1],
 * linN.weight_v [out,in], linN.bias [out]).  With weight_norm == 0, v holds linN.weight and g is
 * ignored. */
typedef struct rnb_mlp_params {
  int32_t n_lin;
  int32_t pad_;
  const float* g[RNB_MAX_LIN];
  const float* v[RNB_MAX_LIN];
  const float* b[RNB_MAX_LIN];
} rnb_mlp_params;

typedef struct rnb_mlp_grads { /* same shapes as rnb_mlp_params, written (not accumulated) */
  int32_t n_lin;
  int32_t pad_;
  float* g[RNB_MAX_LIN];
  float* v[RNB_MAX_LIN];
  float* b[RNB_MAX_LIN];
} rnb_mlp_grads;

int rnb_abi_version(void);
/* Identity of this build of the library: 16 hex digits hashed from every source file and the compiler flags
 * (rnb-neus-fork_amd/buildid.py), or "unknown" for a library built without the project's build script.  Profiles and
 * bench lines carry it, so that stored measurements are only quoted for the build they were taken on.  [ABI 4] */
const char* rnb_build_id(void);
const char* rnb_last_error_string(void);

/* ---- weight norm ------------------------------------------------------------------------------
 * Replaces torch.nn.utils.weight_norm's forward/backward as applied at models/fields.py:72-74 and
 * :168-170.  The forward materialises W = g * v / ||v||_row for every layer of both MLPs into one
 * "packed" buffer (tile-padded, skip-layer 1/sqrt(2) folded in, layout private to the library) that
 * all compute entry points consume; the backward maps a gradient buffer of the same layout back to
 * the leaves. `color`/`color_grads` may be NULL (no_albedo training, exp_runner.py:111-112); `sdf` may be
 * NULL when only the albedo network is evaluated (rnb_color_forward).
 * rnb_packed_floats is the size of `packed` in floats: the fp32 weights plus, behind them, the MFMA-operand mirror of
 * the variant in use (written by rnb_weightnorm_fwd: hi / mid / lo bf16 planes for the default x3 arithmetic, a bf16
 * copy for RNB_VARIANT_BF16).  A gradient buffer (`packed_grad`) needs the same allocation size; only its fp32 part is
 * written and read. */
int rnb_packed_floats(const rnb_model_desc* desc, int64_t* n_floats);
int rnb_weightnorm_fwd(const rnb_model_desc* desc, const rnb_mlp_params* sdf, const rnb_mlp_params* color,
                       float* packed, rnb_stream_t stream);
int rnb_weightnorm_bwd(const rnb_model_desc* desc, const rnb_mlp_params* sdf, const rnb_mlp_params* color,
                       const float* packed_grad, const rnb_mlp_grads* sdf_grads,
                       const rnb_mlp_grads* color_grads, rnb_stream_t stream);

/* ---- point-wise network evaluation (no autograd) ---------------------------------------------
 * rnb_sdf_forward   : SDFNetwork.forward / .sdf      (models/fields.py:82-108)
 *                     sdf_out [n]; feat_out [n, d_out-1] or NULL
 * rnb_sdf_gradient  : SDFNetwork.gradient            (models/fields.py:114-127), grad_out [n,3];
 *                     sdf_out optional
 * rnb_color_forward : RenderingNetwork.forward       (models/fields.py:177-215), out [n, d_out]
 * Used by NeuSRenderer.extract_geometry's query_func (models/renderer.py:1219-1224), by the
 * up-sampling loop and by tests. */
int rnb_points_workspace_bytes(const rnb_model_desc* desc, int64_t n_points, int64_t* bytes);
int rnb_sdf_forward(const rnb_model_desc* desc, const float* packed, const float* pts, int64_t n,
                    float* sdf_out, float* feat_out, void* ws, size_t ws_bytes, rnb_stream_t stream);
int rnb_sdf_gradient(const rnb_model_desc* desc, const float* packed, const float* pts, int64_t n,
                     float* grad_out, float* sdf_out, void* ws, size_t ws_bytes, rnb_stream_t stream);
int rnb_color_forward(const rnb_model_desc* desc, const float* packed, const float* pts,
                      const float* normals, const float* feats, int64_t n, float* out, void* ws,
                      size_t ws_bytes, rnb_stream_t stream);

/* ---- point-wise network calls with autograd (opt-in: SDFNetwork / RenderingNetwork.set_autograd) ----------------
 * Replace autograd through the reference's direct calls: SDFNetwork.forward / .sdf / .sdf_hidden_appearance
 * (models/fields.py:82-112), SDFNetwork.gradient with create_graph=True (:114-127, differentiated once more) and
 * RenderingNetwork.forward (:177-215), as Runner.validate_mesh_texture (exp_runner.py:584-615) or an eikonal term on free
 * points uses them.  The forward keeps the render path's per-point state in `ws`; the backward is the render backward
 * below the composite (FB, RA, the weight gradients, the albedo backward) seeded with the caller's adjoints, plus the
 * input adjoints.  Every adjoint (NULL = zero) may have any scale: the x2h scales are taken from its recorded maximum.
 *   flags                 RNB_POINTS_FEATURE (feat_out / feat_bar), RNB_POINTS_NORMAL (nrm_out / nrm_bar; d sdf / d x),
 *                         RNB_POINTS_COLOR (the albedo-net call); the forward and its backward take the same flags,
 *                         descriptor, n and ws.  Without RNB_POINTS_NORMAL the reverse sweep's state is not kept.
 * rnb_points_grad_workspace_bytes : host function; >= rnb_points_workspace_bytes for the same n
 * rnb_sdf_forward_save  : sdf_out [n]; feat_out [n, d_out-1]; nrm_out [n,3]
 * rnb_sdf_backward      : sdf_bar [n], feat_bar [n, d_out-1], nrm_bar [n,3] -> packed_grad (written, fp32 part of the
 *                         packed layout: rnb_weightnorm_bwd maps it to the leaves) and x_bar [n,3] (NULL: not wanted)
 * rnb_color_forward_save: out [n, d_out] from pts, normals [n,3] and feats [n, d_feature]
 * rnb_color_backward    : alb_bar [n, d_out] -> packed_grad (albedo rows), feat_bar [n, d_feature], nrm_bar [n,3],
 *                         pts_bar [n,3] (each optional).  view_dirs are not an input (mode no_view_dir). */
enum { RNB_POINTS_FEATURE = 1, RNB_POINTS_NORMAL = 2, RNB_POINTS_COLOR = 4 };
int rnb_points_grad_workspace_bytes(const rnb_model_desc* desc, int64_t n_points, int32_t flags, int64_t* bytes);
int rnb_sdf_forward_save(const rnb_model_desc* desc, const float* packed, const float* pts, int64_t n,
                         int32_t flags, float* sdf_out, float* feat_out, float* nrm_out, void* ws, size_t ws_bytes,
                         rnb_stream_t stream);
int rnb_sdf_backward(const rnb_model_desc* desc, const float* packed, int64_t n, int32_t flags, const float* sdf_bar,
                     const float* feat_bar, const float* nrm_bar, float* packed_grad, float* x_bar, void* ws,
                     size_t ws_bytes, rnb_stream_t stream);
int rnb_color_forward_save(const rnb_model_desc* desc, const float* packed, const float* pts, const float* normals,
                           const float* feats, int64_t n, float* out, void* ws, size_t ws_bytes, rnb_stream_t stream);
int rnb_color_backward(const rnb_model_desc* desc, const float* packed, int64_t n, const float* alb_bar,
                       float* packed_grad, float* feat_bar, float* nrm_bar, float* pts_bar, void* ws, size_t ws_bytes,
                       rnb_stream_t stream);

/* ---- SDF grid of validate_mesh --------------------------------------------------------------------
 * extract_fields (models/renderer.py:10-25) with query_func = -sdf_network.sdf (models/renderer.py:1219-1224):
 * volume[ix - x_begin, iy, iz] = out_scale * sdf(X[ix], Y[iy], Z[iz]) for x_begin <= ix < x_end, with
 * X = torch.linspace(bound_min[0], bound_max[0], resolution) etc. generated INSIDE the forward kernel (no point
 * buffer, no per-point workspace for the 256-wide network: 512^3 = 1.3e8 evaluations are one launch).  A rank of
 * a data-parallel job asks for its own x-slab.  volume: device [x_end - x_begin, resolution, resolution]. */
typedef struct rnb_grid_desc {
  float bound_min[3];
  float bound_max[3];
  int32_t resolution;
  int32_t x_begin, x_end;
  float out_scale;        /* -1: the reference negates the SDF */
} rnb_grid_desc;
int rnb_sdf_grid_workspace_bytes(const rnb_model_desc* desc, const rnb_grid_desc* grid, int64_t* bytes);
int rnb_sdf_grid(const rnb_model_desc* desc, const float* packed, const rnb_grid_desc* grid, float* volume,
                 void* ws, size_t ws_bytes, rnb_stream_t stream);

/* ---- sparse SDF grid: only the bricks the iso-surface may pass through are evaluated ------------------
 * The grid is rnb_sdf_grid's (same samples, same index arithmetic, the whole grid: x_begin = 0, x_end = resolution);
 * "inside" is marching cubes' notion, value <= threshold, NaN = outside.
 *   brick   : a cube of `brick`^3 cells, i.e. the (brick+1)^3 samples [b*brick, min((b+1)*brick, res-1)] per axis;
 *             neighbours share their face samples, the last brick per axis may be short; nb = ceil((res-1)/brick) per axis.
 *   lattice : the brick corners, the grid samples min(k*brick, res-1), k = 0..nb — evaluated by the same kernel as the
 *             dense grid, so a lattice value is the very number rnb_sdf_grid writes there.
 *   seeds   : bricks whose 8 corners are not all inside / all outside, or have a non-finite corner, or have a corner with
 *             |value - threshold| < margin * |out_scale| * (half the brick's diagonal in world units).  `margin` is the
 *             Lipschitz constant of the SDF the caller assumes (1 = exact for a true distance field: every point of a cube
 *             is within half a diagonal of a corner; 0 = sign changes only).
 *   growth  : every face of an evaluated brick whose samples are not all inside / all outside lists the brick behind it;
 *             rounds repeat until one lists nothing (at most 3*nb rounds).
 *   volume  : [res,res,res] fp32, dense.  Samples of listed bricks hold the evaluated values, BIT-EQUAL to rnb_sdf_grid's
 *             (same coordinates, same kernel family, rows independent of their tile mates; a tile of the default arithmetic
 *             whose activations outgrow the fixed fp16 scale is rescaled as a whole, which is the one case where tile mates
 *             matter).  Every other sample holds the trilinear interpolant of its brick's 8 lattice values clamped to their
 *             min / max: not an SDF value, but on the corners' side of the threshold and continuous across unlisted faces,
 *             so marching cubes on the volume creates no crossing outside the listed bricks.
 * Guarantee: every iso-surface component that passes through at least one seed brick is reproduced exactly as the dense
 * grid gives it.  A component lying wholly inside bricks whose corners have one sign and are farther than the margin from
 * the threshold is MISSED: raise `margin`, or use rnb_sdf_grid.
 *
 * Calling sequence (no allocation, no synchronisation, the given stream only; the host reads the 8-byte device counter
 * n_listed between calls and sizes the next call from it):
 *   _seed   evaluates the lattice into the workspace, lists the seeds, writes their number to *n_listed;
 *   _round  evaluates the listed bricks [first, first+count) into `volume` (count <= the value read), then grows:
 *           *n_listed becomes the new length of the list; repeat with the new tail until nothing was added;
 *   _finish fills every sample outside the listed bricks; brick_mask (device uint8 [nb,nb,nb], or NULL) gets 1 for listed.
 * The workspace holds the lattice, one state byte per brick and the list (O(nb^3)), plus the per-point buffers of one
 * 2^20-point chunk for shapes on the per-layer route; the same buffer must be passed to all calls of one extraction.
 * RNB_E_INVALID before any launch: an x-slab, brick not in {4, 8, 16, 32}, margin < 0 or NaN, resolution < 2, more than
 * 2^31 - 1 bricks.  RNB_E_WORKSPACE before any launch: ws_bytes below the query's answer. */
typedef struct rnb_sparse_grid_desc {
  int32_t brick;
  float threshold;
  float margin;
} rnb_sparse_grid_desc;
int rnb_sdf_grid_sparse_workspace_bytes(const rnb_model_desc* desc, const rnb_grid_desc* grid,
                                        const rnb_sparse_grid_desc* sparse, int64_t* bytes);
int rnb_sdf_grid_sparse_seed(const rnb_model_desc* desc, const float* packed, const rnb_grid_desc* grid,
                             const rnb_sparse_grid_desc* sparse, void* ws, size_t ws_bytes, int64_t* n_listed,
                             rnb_stream_t stream);
int rnb_sdf_grid_sparse_round(const rnb_model_desc* desc, const float* packed, const rnb_grid_desc* grid,
                              const rnb_sparse_grid_desc* sparse, float* volume, void* ws, size_t ws_bytes, int64_t first,
                              int64_t count, int64_t* n_listed, rnb_stream_t stream);
int rnb_sdf_grid_sparse_finish(const rnb_model_desc* desc, const rnb_grid_desc* grid, const rnb_sparse_grid_desc* sparse,
                               float* volume, void* ws, size_t ws_bytes, uint8_t* brick_mask, rnb_stream_t stream);

/* ---- hierarchical sampling ---------------------------------------------------------------------
 * rnb_up_sample_step: one iteration of the loop at models/renderer.py:970-982 WITHOUT the network
 *   call: NeuSRenderer.up_sample (:132-176) + sample_pdf(det=True) (:39-69) + the concat/sort half of
 *   cat_z_vals (:178-183).  z_in [B,n] sorted, sdf_in [B,n];
 *   outputs new_z [B,n_new], inds int32 [B,n_new] (= torch.searchsorted(cdf,u,right=True)),
 *   z_out [B,n+n_new] sorted, sort_index int32 [B,n+n_new] (= index of torch.sort over cat[z,new_z]).
 * rnb_gather_sdf: sdf_out[b,k] = cat[sdf_old, sdf_new][b, sort_index[b,k]]   (renderer.py:185-190)
 * rnb_sample_rays: the whole no-grad prologue shared by render / render_rnb / render_rnb_warmup
 *   (models/renderer.py:557-608 == :829-880 == :933-984): z = near + (far-near)*linspace(0,1,n_samples)
 *   (+ (t_rand-0.5)*2/n_samples when t_rand != NULL), coarse SDF, up_sample_steps x (up_sample,
 *   cat_z_vals incl. SDF evaluation of the new points).  z_vals_out [B, n_samples+n_importance].
 *   `t_rand` [B] is the torch.rand([B,1]) draw of renderer.py:572, made by the caller.
 * Limits (one wave64 per ray, the ray's depths in LDS): n >= 2, 1 <= n_new <= 64, n + n_new <= 512 per step; for a
 *   descriptor: n_samples >= 2 and, with n_importance > 0, n_importance a multiple of up_sample_steps,
 *   n_importance / up_sample_steps <= min(n_samples, 64) and n_samples + n_importance <= 512.  A descriptor outside
 *   them is refused with RNB_E_INVALID by rnb_sample_workspace_bytes, and by rnb_sample_rays before its first launch. */
int rnb_up_sample_step(const float* rays_o, const float* rays_d, const float* z_in, const float* sdf_in,
                       int64_t B, int32_t n, int32_t n_new, float inv_s, float* new_z, int32_t* inds,
                       float* z_out, int32_t* sort_index, rnb_stream_t stream);
int rnb_gather_sdf(const float* sdf_old, const float* sdf_new, const int32_t* sort_index, int64_t B,
                   int32_t n, int32_t n_new, float* sdf_out, rnb_stream_t stream);
int rnb_sample_workspace_bytes(const rnb_model_desc* desc, int64_t B, int64_t* bytes);
int rnb_sample_rays(const rnb_model_desc* desc, const float* packed, const float* rays_o,
                    const float* rays_d, const float* near, const float* far, const float* t_rand,
                    int64_t B, float* z_vals_out, void* ws, size_t ws_bytes, rnb_stream_t stream);

/* ---- fine pass: render cores + wrappers ---------------------------------------------------------
 * rnb_render_fwd evaluates NeuSRenderer.render_core (models/renderer.py:194-285; mode RNB_MODE_CORE,
 * the composite of NeuSRenderer.render :632-648) or render_core_mvps (:466-554) followed by the
 * multi-light shading composite of render_rnb (:1009-1033; RNB_MODE_MVPS) / render_rnb_warmup
 * (:905-930; RNB_MODE_MVPS | RNB_FLAG_RELU_SHADING) on given sorted z_vals, and keeps what the
 * backward needs in `ws`.  rnb_render_bwd is loss.backward() through that graph
 * (exp_runner.py:261): it consumes gradients w.r.t. the returned tensors and writes gradients w.r.t.
 * the packed weights and the variance scalar. */
enum {
  RNB_MODE_CORE = 0,            /* render(): colour = sum_s c*w (+ background_rgb) */
  RNB_MODE_MVPS = 1,            /* render_rnb*: colour[l] = sum_s albedo*w*(n.l)    */
  RNB_FLAG_RELU_SHADING = 2,    /* warm-up: relu on n.l (renderer.py:913)           */
  RNB_FLAG_NO_ALBEDO = 4,       /* albedo := 1 (renderer.py:905-906, :1009-1010)    */
  RNB_FLAG_LIGHT_PER_RAY = 8,   /* lights_dir is [L,B,3] instead of [L,3]           */
  RNB_FLAG_FORWARD_ONLY = 16,   /* no backward will follow                          */
  RNB_FLAG_INPUT_GRADS = 32     /* keep what rnb_render_bwd_inputs needs (below)    */
};

typedef struct rnb_render_args {
  int64_t B;              /* rays */
  int32_t S;              /* samples per ray (n_samples + n_importance) */
  int32_t n_lights;       /* L (MVPS) ; ignored for CORE */
  int32_t flags;          /* RNB_MODE_* | RNB_FLAG_* */
  float   cos_anneal_ratio;
  const float* rays_o;    /* [B,3] */
  const float* rays_d;    /* [B,3] */
  const float* z_vals;    /* [B,S] sorted */
  const float* lights_dir;/* [L,3] or [L,B,3] */
  const float* background_rgb; /* [3] or NULL (CORE only, renderer.py:266-267) */
  const float* variance;  /* [1] SingleVarianceNetwork.variance (models/fields.py:317-325) */
  /* outputs (keys of the dict returned at renderer.py:638-648 / :1023-1033) */
  float* color_fine;      /* MVPS: [L,B,C]  CORE: [B,3] ; C = col_d_out */
  float* weights;         /* [B,S] */
  float* cdf_fine;        /* [B,S] */
  float* gradients;       /* [B,S,3] */
  float* inside_sphere;   /* [B,S] */
  float* weight_sum;      /* [B] */
  float* weight_max;      /* [B] */
  float* s_val;           /* [B] */
  float* gradient_error;  /* [1] */
  /* optional extra outputs of the cores (may be NULL) */
  float* sdf;             /* [B*S] */
  float* sampled_albedo;  /* [B*S,C] (network output, before the no_albedo override) */
  /* data parallelism with the exact large-batch loss: the eikonal term of models/renderer.py:538-540 is
   * a ratio of two batch-global sums.  rnb_render_fwd writes this shard's sums (numerator, count) to
   * gerr_partial [2] when it is non-NULL; rnb_render_bwd divides by *gerr_den_global (the all-reduced count + 1e-5)
   * instead of the shard's own denominator when it is non-NULL.  Both NULL: single-process behaviour. */
  float* gerr_partial;
  const float* gerr_den_global;
} rnb_render_args;

typedef struct rnb_render_grads { /* d loss / d <output>; NULL = zero */
  const float* color_fine;
  const float* weights;
  const float* cdf_fine;
  const float* gradients;
  const float* weight_sum;
  const float* weight_max;
  const float* s_val;
  const float* gradient_error;
} rnb_render_grads;

/* Limits: 1 <= S <= 512 samples per ray, n_lights <= 8 (RNB_MODE_MVPS).  rnb_render_workspace_bytes refuses a larger S,
 * rnb_render_fwd / rnb_render_bwd / rnb_render_bwd_inputs refuse a larger S or light count (RNB_E_INVALID) before they
 * launch anything. */
int rnb_render_workspace_bytes(const rnb_model_desc* desc, int64_t B, int32_t S, int32_t flags,
                               int64_t* bytes);
int rnb_render_fwd(const rnb_model_desc* desc, const float* packed, const rnb_render_args* args,
                   void* ws, size_t ws_bytes, rnb_stream_t stream);
int rnb_render_bwd(const rnb_model_desc* desc, const float* packed, const rnb_render_args* args,
                   const rnb_render_grads* gout, float* packed_grad, float* variance_grad, void* ws,
                   size_t ws_bytes, rnb_stream_t stream);

/* Gradients with respect to the render's floating-point INPUTS (the reference's autograd reaches every input that requires
 * grad, models/renderer.py:209-272, :478-540, :905-914, :1009-1017):
 *   rays_o [B,3], rays_d [B,3]   through pts = o + d * mid_z into sdf(pts), the normal (its Hessian-vector term included,
 *                                models/fields.py:114-127) and the albedo net's encoded points and normals; rays_d also
 *                                through true_cos = d . n
 *   lights_dir [L,3] | [L,B,3]   through the shading n . l (with the warm-up's ReLU mask); MVPS only
 *   background_rgb [3]           through colour += bg * (1 - sum w); CORE only
 *   z_vals [B,S]                 through dists (the last one is the constant sample_dist) and mid_z
 * A NULL field is "not wanted"; every other field is OVERWRITTEN (not accumulated).  Shared lights and the background are
 * sums over the rays in a fixed order (no floating-point atomics: bit-reproducible). */
typedef struct rnb_render_input_grads {
  float* rays_o;
  float* rays_d;
  float* lights_dir;
  float* background_rgb;
  float* z_vals;
} rnb_render_input_grads;

/* Everything rnb_render_bwd does (same packed_grad and variance_grad), plus the input gradients `igrads` asks for.  The
 * forward must have been made with RNB_FLAG_INPUT_GRADS in args->flags: it then keeps d sdf / d e of the normal's sweep
 * (the Hessian term) and the workspace holds the per-ray partial sums (rnb_render_workspace_bytes with the flag is never
 * smaller than without it).  Lights or background alone do not run the point-wise input adjoint.  Returns RNB_E_INVALID
 * for RNB_VARIANT_BF16 (the flag is refused by the workspace query and the forward too), for a request on a forward made
 * without the flag, for lights in RNB_MODE_CORE and for the background in RNB_MODE_MVPS or without a background.
 * igrads == NULL or all fields NULL: exactly rnb_render_bwd. */
int rnb_render_bwd_inputs(const rnb_model_desc* desc, const float* packed, const rnb_render_args* args,
                          const rnb_render_grads* gout, const rnb_render_input_grads* igrads, float* packed_grad,
                          float* variance_grad, void* ws, size_t ws_bytes, rnb_stream_t stream);

/* ---- whole-image rendering ------------------------------------------------------------------------
 * rnb_render_maps: a forward-only render that returns per-ray IMAGES instead of the training dictionary — what
 * validate_image (exp_runner.py:460-470) reduces from weights / gradients / inside_sphere with torch ops per batch, plus
 * the albedo and depth maps.  Same inputs, modes, flags and limits as rnb_render_fwd (a larger S or light count is refused
 * with the same messages before any launch) and the same launches up to the composite, so for the same inputs color,
 * weight_sum and weight_max are bit-equal to rnb_render_fwd's.  No [B,S] array is written: the per-sample output pointers
 * of `args` are ignored (they may be NULL).  Always forward-only: the workspace is the one
 * rnb_render_workspace_bytes(desc, B, S, flags | RNB_FLAG_FORWARD_ONLY) sizes, RNB_FLAG_INPUT_GRADS is RNB_E_INVALID.
 * Every map is optional (NULL = not wanted); all NULL is RNB_E_INVALID. */
typedef struct rnb_render_maps_out {
  float* color;       /* MVPS: [L,B,C]  CORE: [B,3] (background included): color_fine of the wrapper */
  float* normal;      /* [B,3]  sum_s w_s n_s [|p_s| < 1]                                            */
  float* albedo;      /* [B,C]  sum_s w_s albedo_s ; MVPS with the albedo network only, else RNB_E_INVALID */
  float* depth;       /* [B]    sum_s w_s (z_s + dists_s / 2)                                        */
  float* weight_sum;  /* [B] */
  float* weight_max;  /* [B] */
} rnb_render_maps_out;
int rnb_render_maps(const rnb_model_desc* desc, const float* packed, const rnb_render_args* args,
                    const rnb_render_maps_out* maps, void* ws, size_t ws_bytes, rnb_stream_t stream);

/* Name/duration of the heaviest kernel family, for bench.py's roofline line: fills `flops` with the
 * algorithmic MLP FLOPs of one rnb_render_fwd+bwd (+ sampling) at the given shape. */
int rnb_algorithmic_flops(const rnb_model_desc* desc, int64_t B, int32_t flags, double* train_flops,
                          double* forward_flops);

/* Algorithmic HBM bytes of the per-point saved state one training step (rnb_render_fwd + rnb_render_bwd) moves when
 * every saved matrix is written once and read once by each kernel that consumes it — the traffic floor of the
 * "store, don't recompute" design, which is what bounds the RNB_VARIANT_BF16 step.  Per point:
 * SDF sweeps 15 * n_layers * d_hidden elements (6 matrices written, 9 matrix reads per layer; 2 bytes each with
 * RNB_VARIANT_BF16, else 4) + the albedo network's fp32 activations. */
int rnb_algorithmic_bytes(const rnb_model_desc* desc, int64_t B, int32_t flags, double* train_bytes);

/* ---- Marching cubes of validate_mesh --------------------------------------------------------------
 * Replaces `mcubes.marching_cubes(u, threshold)` (models/renderer.py:31 inside extract_geometry :27-36; called by
 * validate_mesh, exp_runner.py:561-581) on a volume resident in device memory: volume [nx, ny, nz] fp32, C order (the
 * array extract_fields returns).  PyMCubes (third party, un-vendored, not importable here) is the arithmetic being
 * replaced: PARITY UNPINNED; kept from its published behaviour are the classic corner / edge numbering, "inside" :=
 * value <= threshold, ONE vertex per crossed grid edge shared by the cells around it, linear interpolation in double
 * precision and vertices in grid-index coordinates (the caller rescales them, models/renderer.py:34).  Triangles are
 * oriented so that their right-hand normal points towards smaller values.  NaN samples count as outside; an edge
 * between a NaN and an inside sample yields a NaN vertex.
 * Two calls, because the output sizes are data dependent:
 *   rnb_marching_cubes_count  fills counts[0..1] (device int64: vertices, triangles) and the workspace;
 *   -- the caller reads counts, allocates vertices [n_vertices, 3] double and triangles [n_triangles, 3] int32 --
 *   rnb_marching_cubes_emit   same volume / threshold / workspace; writes both arrays.  Deterministic order: vertices
 *                             by owning grid point (x slowest) then edge axis; triangles by cell, then table order.
 * Fails with RNB_E_INVALID beyond 2^30 vertices (vertex ids are 30-bit) or 2^32 grid points. */
int rnb_marching_cubes_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t* bytes);
int rnb_marching_cubes_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, float threshold,
                             void* workspace, size_t workspace_bytes, int64_t* counts, rnb_stream_t stream);
int rnb_marching_cubes_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, float threshold,
                            void* workspace, size_t workspace_bytes, int64_t n_vertices, int64_t n_triangles,
                            double* vertices, int32_t* triangles, rnb_stream_t stream);

/* ---- Per-vertex attributes of validate_mesh_texture --------------------------------------------------
 * What Runner.validate_mesh_texture (exp_runner.py:584-625) computes for every mesh vertex with sdf_network(v),
 * sdf_network.gradient(v) and color_network(v, g, g, feat) in chunks on the host side: SDF, gradient, unit normal, albedo
 * and the 8-bit vertex colour, for ANY number of vertices, in one call on the device.
 * Vertices come either as `grid_vertices` (float64 grid-index coordinates, the array rnb_marching_cubes_emit writes; they
 * are rescaled to the bounding box as models/renderer.py:34 does, then rounded to fp32:
 *     p = (float)(v / (resolution - 1.0) * (double)(bound_max - bound_min) + (double)bound_min),
 * bound_max - bound_min taken in fp32, multiply and add unfused — bit for bit the host's numpy expression followed by
 * torch's conversion to float32) or as fp32 model-space `points` (copied).
 * The library loops over chunks of `chunk` vertices (a positive multiple of 64) through ONE workspace of
 * rnb_mesh_vertex_workspace_bytes(desc, chunk, flags) bytes, whatever V (stream order makes the reuse safe).  Per chunk:
 * forward sweep (state saved) + reverse sweep on the model's kernel route; `refine` Newton steps towards the level set
 *     p <- p - t g,   t = (sdf - level) / |g|^2,   displacement |t| |g| clamped to max_step,
 * each followed by the two sweeps again (a point whose sdf or g is not finite, or with |g|^2 < 1e-12, is left where it
 * is; max_step bounds the distance between the stored fp32 points, so the clamp is max_step less half an ulp of every
 * coordinate); the albedo network ONCE at the final points, with g as its normal input, when RNB_MESH_ALBEDO is set; one epilogue
 * kernel that writes the requested outputs.  Nothing is launched for V == 0.
 *   rgb_out = (uint8) rintf(255 * min(max(a, 0), 1)) in fp32, channel order [2,1,0] with RNB_MESH_SWAP_RB (the reference's
 *   BGR -> RGB swap); col_d_out == 1 replicates the one channel.
 * RNB_E_INVALID before any launch: chunk not a positive multiple of 64; unknown flag bits; RNB_MESH_ALBEDO on a model
 * without an albedo network; albedo_out or rgb_out without RNB_MESH_ALBEDO; rgb_out with col_d_out other than 1 or 3;
 * refine < 0, or refine > 0 with max_step <= 0; V < 0; grid_vertices with resolution < 2; every output pointer NULL.
 * RNB_E_NULL: both grid_vertices and points NULL (V > 0).  RNB_E_WORKSPACE: ws_bytes below the query's answer. */
enum { RNB_MESH_ALBEDO = 1, RNB_MESH_SWAP_RB = 2 };
typedef struct rnb_mesh_vertex_args {
  const double* grid_vertices;  /* [V,3] grid-index coordinates as rnb_marching_cubes_emit writes them, or NULL */
  const float* points;          /* [V,3] model-space points; read when grid_vertices is NULL */
  int64_t V;
  float bound_min[3], bound_max[3];
  int32_t resolution;           /* bounds and resolution: used with grid_vertices only */
  float level;                  /* SDF value of the surface: -threshold (the volume holds -sdf) */
  int32_t refine;               /* Newton steps (0: evaluate where the vertices are) */
  float max_step;               /* largest displacement of one Newton step (model units) */
  int32_t flags;                /* RNB_MESH_* */
  float* points_out;            /* [V,3] the points the attributes were evaluated at (after refinement) */
  float* sdf_out;               /* [V] */
  float* gradient_out;          /* [V,3] d sdf / d x, unnormalised (what the reference feeds the albedo net) */
  float* normal_out;            /* [V,3] gradient / |gradient|; (0,0,0) where |gradient| is 0 or not finite */
  float* albedo_out;            /* [V,col_d_out] raw network output */
  uint8_t* rgb_out;             /* [V,3] */
} rnb_mesh_vertex_args;         /* every output pointer may be NULL; at least one must not be */
int rnb_mesh_vertex_workspace_bytes(const rnb_model_desc* desc, int64_t chunk, int32_t flags, int64_t* bytes);
int rnb_mesh_vertex_attrs(const rnb_model_desc* desc, const float* packed, const rnb_mesh_vertex_args* args,
                          int64_t chunk, void* ws, size_t ws_bytes, rnb_stream_t stream);

/* ---- Mesh cleanup: connected components, per-component statistics, compaction ----------------------------
 * The first thing done to a marching-cubes mesh after validate_mesh: keep the largest connected component, or drop the
 * small ones (floaters, shell fragments at the box walls) — on the arrays rnb_marching_cubes_emit left in device memory.
 *   triangles [T,3] int32, vertices [V,3] float64 (any coordinates), 0 <= V, T <= 2^31 - 1.
 * Two vertices are connected when some triangle names both (degenerate triangles count like any other); a component is a
 * class of the transitive closure over the vertices at least one triangle names.  Components are numbered 0 .. C-1 in
 * increasing order of their smallest vertex index — independent of the schedule.  A vertex no triangle names is
 * unreferenced: label -1, in no component, never kept.
 * Every stage works in ONE workspace of rnb_mesh_clean_workspace_bytes(V, T) bytes (a stage may overwrite what the
 * previous one left there, except that rnb_mesh_compact_emit reads what rnb_mesh_compact_count wrote).
 *   rnb_mesh_components       labels [V] int32; counts[0] = C, counts[1] = 1 when some triangle holds an index outside
 *                             [0, V) (device int64 [2]).  Such a triangle is skipped — every index is checked before it
 *                             is used as an address — and the caller should treat the mesh as invalid.
 *                             Lock-free union-find, one thread per triangle, the larger root hooked under the smaller
 *                             (csrc/mesh_clean.hip has the termination argument: parent[x] <= x always).
 *   -- the caller reads counts and allocates the [C] arrays --
 *   rnb_mesh_component_stats  tri_count [C], vert_count [C] int64; with vertices != NULL also area [C] float64, the sum
 *                             of 0.5 |(p1 - p0) x (p2 - p0)| over the component's triangles, and bbox_min / bbox_max
 *                             [C,3] float64, the exact minimum / maximum.  No floating-point atomics: the area is
 *                             accumulated as a 128-bit integer in units of 2^-54 of the power of two at or below the
 *                             component's largest triangle (each triangle rounded to that unit: at most 2^-55 of the
 *                             largest per triangle), so it is bit-reproducible from run to run.  A component with a NaN
 *                             coordinate has NaN in that axis of its bbox, and a NaN area when the NaN reaches a triangle.
 *   rnb_mesh_compact_count    keep [C] uint8 (device; non-zero = keep the component); counts[0] = kept vertices V',
 *                             counts[1] = kept triangles T' (device int64 [2])
 *   -- the caller reads counts and allocates the outputs --
 *   rnb_mesh_compact_emit     vertices_out [V',3] (written when vertices != NULL), triangles_out [T',3] with the indices
 *                             remapped, vertex_index [V'] int64 = the old index of every kept vertex.  Stable: kept
 *                             vertices and triangles keep their relative order, triangles their corner order.
 * RNB_E_INVALID before any launch: V or T negative or above 2^31 - 1, n_components outside [0, V], output sizes above
 * the input sizes.  RNB_E_NULL: a required pointer is NULL.  RNB_E_WORKSPACE: workspace_bytes below the query's answer. */
int rnb_mesh_clean_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes);
int rnb_mesh_components(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                        size_t workspace_bytes, int32_t* labels, int64_t* counts, rnb_stream_t stream);
int rnb_mesh_component_stats(const int32_t* triangles, int64_t n_triangles, const double* vertices, int64_t n_vertices,
                             const int32_t* labels, int64_t n_components, void* workspace, size_t workspace_bytes,
                             int64_t* tri_count, int64_t* vert_count, double* area, double* bbox_min, double* bbox_max,
                             rnb_stream_t stream);
int rnb_mesh_compact_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* labels,
                           const uint8_t* keep, int64_t n_components, void* workspace, size_t workspace_bytes,
                           int64_t* counts, rnb_stream_t stream);
int rnb_mesh_compact_emit(const int32_t* triangles, int64_t n_triangles, const double* vertices, int64_t n_vertices,
                          const int32_t* labels, const uint8_t* keep, int64_t n_components, void* workspace,
                          size_t workspace_bytes, int64_t n_vertices_out, int64_t n_triangles_out, double* vertices_out,
                          int32_t* triangles_out, int64_t* vertex_index, rnb_stream_t stream);

/* Compaction by a per-triangle keep (what survives a culling, rnb_mesh_view_votes below): the two calls above with
 * another rule of what is kept, in the same workspace of rnb_mesh_clean_workspace_bytes(V, T) bytes.
 *   keep_t [T] uint8 (device).  A triangle is KEPT when keep_t[t] != 0 and its three indices lie in [0, V) — every index
 *   is checked before it is used as an address; a vertex is KEPT when a kept triangle names it.
 *   rnb_mesh_compact_triangles_count   counts[0] = V', counts[1] = T' (device int64 [2])
 *   -- the caller reads counts and allocates the outputs --
 *   rnb_mesh_compact_triangles_emit    as rnb_mesh_compact_emit (stable order, indices remapped, vertex_index [V'] int64),
 *                                      and triangle_index [T'] int64 = the old index of every kept triangle.  Same mesh,
 *                                      keep_t and workspace size as the count, whose block sums it reads.
 * Errors as for rnb_mesh_compact_count / _emit. */
int rnb_mesh_compact_triangles_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                     const uint8_t* keep_t, void* workspace, size_t workspace_bytes, int64_t* counts,
                                     rnb_stream_t stream);
int rnb_mesh_compact_triangles_emit(const int32_t* triangles, int64_t n_triangles, const double* vertices,
                                    int64_t n_vertices, const uint8_t* keep_t, void* workspace, size_t workspace_bytes,
                                    int64_t n_vertices_out, int64_t n_triangles_out, double* vertices_out,
                                    int32_t* triangles_out, int64_t* vertex_index, int64_t* triangle_index,
                                    rnb_stream_t stream);

/* ---- Mesh simplification: vertex clustering on a uniform grid, to a cell size ------------------------------
 * Makes a marching-cubes mesh smaller on the device (Rossignac-Borrel): the vertices of one grid cell become one vertex,
 * which is ONE OF THEM (the member nearest the cell's mean), so every output vertex is an input vertex, per-vertex
 * attributes carry over by a gather, and the result is defined bit for bit (tests/mesh_simplify_ref.py restates it in numpy).
 *   vertices [V,3] float64, triangles [T,3] int32, 0 <= V, T <= 2^31 - 1; the grid: origin[3] (finite; host memory, or
 *   NULL = per axis the minimum over the vertices whose three coordinates are finite, computed on the device; 0 when there
 *   is none) and cell_size h (positive, finite).  The grid is unbounded, nothing is clamped, there is no per-cell array.
 * Definition.
 *   Cell of a coordinate   u = (x - origin) / h (two roundings), i = floor(u), f = u - i (exact, except that a negative u
 *                          of tiny magnitude gives f = 1).  A vertex is USABLE when its three coordinates are finite and
 *                          every i lies in [-2^20, 2^20); its cell key is (ix + 2^20) | (iy + 2^20) << 21 | (iz + 2^20) << 42.
 *   Valid triangle         all three indices in [0, V) — every index is checked before it is used as an address — and all
 *                          three vertices usable.  Any other triangle is skipped.  A vertex is REFERENCED when a valid
 *                          triangle names it; only referenced vertices take part in anything below.
 *   Cluster                the referenced vertices of one cell; its LEADER is its smallest vertex index.
 *   Cluster mean           in cell units, from integer sums (independent of the order of accumulation): per axis
 *                          q = (uint64) floor(f * 2^32), S = sum of q over the n members (64-bit), m = ((double) S /
 *                          (double) n) * 2^-32.
 *   Representative         the member that minimises (d2, vertex index) lexicographically, d2 = ((fx - mx)^2 + (fy - my)^2)
 *                          + (fz - mz)^2 with every operation rounded on its own (d2 >= 0: its bits order as an integer).
 *   Triangles              a valid triangle maps to the clusters of its corners, corner order kept.  It is DEGENERATE when
 *                          two corners share a cluster: dropped.  Among the others, those with the same UNORDERED cluster
 *                          triple are duplicates whatever their orientation: the one with the smallest input index survives.
 *   Output                 surviving triangles in input order; the clusters at least one surviving triangle names, numbered
 *                          in increasing order of leader; vertices_out[j] = vertices[representative of cluster j], bit for bit.
 * Two calls in ONE workspace of rnb_mesh_simplify_workspace_bytes(V, T) bytes (a host function, monotone in both):
 *   rnb_mesh_simplify_count  counts (device int64 [6]): [0] = V', [1] = T', [2] = degenerate triangles, [3] = duplicates
 *                            removed ([1] + [2] + [3] = valid triangles), [4] = flag bits: 1 = a triangle was skipped for an
 *                            index outside [0, V), 2 = one was skipped for a vertex that is not usable (4 = a table filled
 *                            up, which its sizing excludes), [5] = clusters.
 *   -- the caller reads counts and allocates the outputs --
 *   rnb_mesh_simplify_emit   reads what the count left in the workspace: same mesh, same grid, same workspace size.
 *                            vertices_out [V',3], triangles_out [T',3] int32, vertex_index [V'] int64 = the input index of
 *                            every output vertex, vertex_cluster [V] int32 = the output index of every input vertex's
 *                            cluster (-1: unreferenced, or its cluster is not in the output), triangle_index [T'] int64 =
 *                            the input index of every surviving triangle.  vertex_cluster and triangle_index may be NULL.
 * Two open-addressing tables of 32-bit slots (cells -> leader, cluster triples -> first triangle; csrc/mesh_simplify.hip
 * has the argument why an insertion ends and a key ends in exactly one slot), integer atomics only, no floating-point
 * atomic: the result does not depend on the schedule.
 * RNB_E_INVALID before any launch: V or T negative or above 2^31 - 1, cell_size not positive and finite, origin not finite,
 * output sizes above the input sizes.  RNB_E_NULL: a required pointer is NULL.  RNB_E_WORKSPACE: workspace_bytes below the
 * query's answer.  Nothing is launched for T == 0: counts are zero, vertex_cluster is -1.  Nothing is allocated and no
 * device-wide synchronisation happens inside these calls. */
int rnb_mesh_simplify_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes);
int rnb_mesh_simplify_count(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                            const double* origin, double cell_size, void* workspace, size_t workspace_bytes,
                            int64_t* counts, rnb_stream_t stream);
int rnb_mesh_simplify_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                           const double* origin, double cell_size, void* workspace, size_t workspace_bytes,
                           int64_t n_vertices_out, int64_t n_triangles_out, double* vertices_out, int32_t* triangles_out,
                           int64_t* vertex_index, int32_t* vertex_cluster, int64_t* triangle_index, rnb_stream_t stream);

/* ---- Mesh topology audit: edges, boundaries, watertightness ---------------------------------------------------
 * What the stages that change connectivity (culling, clustering, a surface that leaves the box) did to a mesh: is it closed,
 * how many holes, is it oriented consistently — on the device, defined bit for bit (tests/mesh_topology_ref.py restates it
 * in numpy).
 *   triangles [T,3] int32, V vertices, optionally vertices [V,3] float64; 0 <= V <= 2^31 - 1, 0 <= T <= 1,431,655,764
 *   (3 T <= 2^32 - 4: a half-edge index fits a 32-bit table slot).
 * Definition.
 *   Triangle classes    INVALID: an index outside [0, V) — every index is checked before it is used as an address.  A valid
 *                       triangle is DEGENERATE when two of its indices are equal.  The others are PROPER: only they have edges.
 *   Half-edges          proper triangle t = (a, b, c) has the half-edges 3t + 0 = (a, b), 3t + 1 = (b, c), 3t + 2 = (c, a).
 *   Edge key            the undirected edge of half-edge (p, q) has the key min(p, q) * 2^31 + max(p, q); the half-edge is
 *                       FORWARD when p < q, else BACKWARD.  n_fwd / n_bwd of an edge count its forward / backward half-edges.
 *   Edge classes        BOUNDARY n_fwd + n_bwd == 1; MANIFOLD n_fwd == n_bwd == 1; FLIPPED (2, 0) or (0, 2): two triangles
 *                       that disagree about the orientation; NON-MANIFOLD three or more uses.
 *   Leader              the smallest half-edge index of an edge.  Edges are listed in increasing order of leader (no sort).
 *   Triangle flags      uint8: 1 = has a boundary edge, 2 = a flipped edge, 4 = a non-manifold edge, 8 = degenerate, 16 = invalid.
 *   Vertex flags        uint8: 1 = on a boundary edge, 2 = on a flipped edge, 4 = on a non-manifold edge, 8 = named by no
 *                       proper triangle.
 *   Boundary components the classes of the transitive closure over the vertices a boundary edge joins, numbered in increasing
 *                       order of their smallest vertex; boundary_labels[v] = -1 off the boundary.  boundary_degree[v] = the
 *                       number of boundary edges at v; the boundary is SIMPLE when that is 2 at every boundary vertex: then
 *                       every boundary component is one closed loop, one hole.
 *   Component table     per component of rnb_mesh_components' labels (unchanged), int64 [C,8]: [0..3] boundary, manifold,
 *                       flipped, non-manifold edges (an edge belongs to the component of its smaller vertex), [4] proper and
 *                       [5] degenerate triangles (the component of the first corner), [6] boundary components (that of their
 *                       smallest vertex; -1 when the count made none), [7] vertices a proper triangle names.
 *   Signed volume       with vertices: the sum over the component's proper triangles of term = (((x0 cx + y0 cy) + z0 cz) / 6),
 *                       cx = y1 z2 - z1 y2, cy = z1 x2 - x1 z2, cz = x1 y2 - y1 x2, every product, sum and the division
 *                       rounded on its own.  Accumulated like the area of rnb_mesh_component_stats, signed: a 128-bit
 *                       two's-complement integer in units of 2^(e_c - 54), e_c the exponent of the component's largest |term|
 *                       (each term rounded to that unit: at most 2^-55 of the largest per triangle), converted with one
 *                       rounding — bit-reproducible from run to run, no floating-point atomic.  NaN when a proper triangle
 *                       of the component has a non-finite corner or a non-finite term.  It is the ENCLOSED volume only for
 *                       a closed, consistently oriented component; its sign is the orientation (positive: counter-clockwise
 *                       seen from outside).
 *   NOT detected        vertex-manifoldness: a vertex where two fans touch (a "bow-tie") has only manifold edges.  Duplicate
 *                       triangles show only through their edges (non-manifold, or flipped for a reversed copy of a
 *                       boundary triangle).
 * Three calls in ONE workspace of rnb_mesh_topology_workspace_bytes(V, T) bytes (a host function of the sizes alone):
 *   rnb_mesh_topology_count       counts (device int64 [8]): E, boundary, manifold, flipped, non-manifold edges, degenerate
 *                                 triangles, invalid triangles, boundary components; tri_flags [T], vert_flags [V];
 *                                 boundary_labels [V] and boundary_degree [V] int32, both given or both NULL: with NULL no
 *                                 boundary component is made and counts[7] = -1.  (counts[0] = -1: the edge table filled up,
 *                                 which its sizing excludes.)
 *   -- the caller reads counts and allocates the outputs --
 *   rnb_mesh_topology_emit        same mesh and workspace, reading what the count left: edges [E,2] int32 (min, max), edge_use
 *                                 [E,2] int32 (n_fwd, n_bwd), edge_triangle [E] int32 (the leader's triangle), in leader order.
 *   rnb_mesh_topology_components  labels [V], C of rnb_mesh_components and the workspace of the count: table [C,8] int64 and,
 *                                 with vertices != NULL, volume [C] float64.  It leaves what the emit reads alone.
 * The edge table is the open-addressing table of the simplification (32-bit slots holding a half-edge index, two slots per
 * half-edge, the argument in csrc/mesh_simplify.hip), the boundary components the lock-free union-find of the cleanup;
 * integer atomics only: no result depends on the schedule.
 * RNB_E_INVALID before any launch: V or T out of range, n_edges outside [0, 3T], n_components outside [0, V].  RNB_E_NULL: a
 * required pointer (the workspace included) is NULL.  RNB_E_WORKSPACE: workspace_bytes below the query's answer.  Nothing is
 * allocated and no device-wide synchronisation happens inside these calls. */
int rnb_mesh_topology_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes);
int rnb_mesh_topology_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                            size_t workspace_bytes, int64_t* counts, uint8_t* tri_flags, uint8_t* vert_flags,
                            int32_t* boundary_labels, int32_t* boundary_degree, rnb_stream_t stream);
int rnb_mesh_topology_emit(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* workspace,
                           size_t workspace_bytes, int64_t n_edges, int32_t* edges, int32_t* edge_use, int32_t* edge_triangle,
                           rnb_stream_t stream);
int rnb_mesh_topology_components(const int32_t* triangles, int64_t n_triangles, const double* vertices, int64_t n_vertices,
                                 const int32_t* labels, int64_t n_components, void* workspace, size_t workspace_bytes,
                                 int64_t* table, double* volume, rnb_stream_t stream);

/* ---- Mesh hole filling: ordered boundary loops, fan caps ------------------------------------------------------------
 * What closes the holes the audit above reports (csrc/mesh_fill.hip; tests/mesh_fill_ref.py restates it in numpy): the
 * boundary components as ordered polygons, and a fan of triangles around the centroid of every loop that can be walked.
 *   Sizes as for the audit: 0 <= V <= 2^31 - 1, 0 <= T <= 1,431,655,764 (half-edge indices are 32-bit).
 * Definition.
 *   Boundary half-edge  the single use of a BOUNDARY edge: the half-edge p -> q of a proper triangle whose edge no other
 *                       half-edge uses.  Invalid and degenerate triangles have none.
 *   Loops               the boundary components of rnb_mesh_topology_count, in its numbering (by smallest vertex); loop l has
 *                       the vertices with boundary_labels == l.
 *   Status              0 SIMPLE: every vertex of the loop has boundary_degree 2, one outgoing and one incoming boundary
 *                       half-edge: the loop is one closed polygon.  1 TANGLED: some vertex has boundary_degree != 2 (two
 *                       holes that touch).  2 MISORIENTED: degree 2 everywhere, but some vertex has two outgoing or two
 *                       incoming half-edges (the surface changes orientation along the hole).
 *   loop_edges          the boundary edges of the loop: half the sum of its vertices' boundary degrees (= its number of
 *                       vertices when it is SIMPLE).
 *   Ordered loops       CSR: loop_offsets [L + 1] int64, loop_vertices [B] int32, B = the number of boundary vertices.  A SIMPLE
 *                       loop of n vertices w[0..n): w[0] = its smallest vertex, w[j + 1] = the head of the boundary half-edge
 *                       that leaves w[j].  A loop of another status lists its vertices in increasing index; it is not walked.
 *   Loop mean           per loop and column the mean of a per-vertex array over the loop's vertices: every value enters a
 *                       128-bit integer sum in units of 2^(e - 54), e the exponent of the largest |value| of that loop and
 *                       column (an error of at most 2^-55 of the largest per vertex), the sum is converted with one rounding
 *                       and divided by n in fp64; for float32 values the quotient is then rounded once to float32.  Integer
 *                       atomics only: bit-equal from run to run.  NaN when a value of the loop is not finite.  The loop
 *                       centroid is the loop mean of the vertex positions.
 *   The cap             a loop is FILLED when it is SIMPLE and has at most max_edges edges (max_edges < 0: no limit).  The
 *                       filled loops are ranked r = 0 .. F - 1 in loop order.  Loop r adds vertex V + r at its centroid and the
 *                       n triangles (w[(j + 1) mod n], w[j], V + r), j = 0 .. n - 1, appended in that order, loop after loop,
 *                       behind the T old triangles; old vertices and triangles are copied bit for bit, invalid and degenerate
 *                       triangles and unreferenced vertices included.  Each rim edge is used once against its one existing
 *                       use, so the cap inherits the surface's orientation.
 * The calls, in the count / emit idiom.  A departure from one count and one emit over one workspace: the loops are found from
 * what rnb_mesh_topology_count left — its workspace (read, never written) and its boundary_labels / boundary_degree — so
 * the edge table is built once for an audit and a fill; and the means are a call of their own, which serves the centroid
 * and any number of attribute arrays.  The fill's own workspace has rnb_mesh_fill_workspace_bytes(V, T) bytes.
 *   rnb_mesh_loops_count  after rnb_mesh_topology_count on the same mesh with boundary arrays.  counts (device int64 [16]):
 *                         [0] L loops, [1] B boundary vertices, [2] F filled loops, [3] N new triangles, [4] TANGLED,
 *                         [5] MISORIENTED loops, [6] SIMPLE loops with more than max_edges edges, [7] the longest filled loop,
 *                         [8] the longest SIMPLE loop, [9] the vertices of loops that are not SIMPLE, [10] -1 when the audit's
 *                         edge table had filled up or a value was out of range (its sizing excludes both), [11..15] 0.
 *   -- the caller reads counts and allocates the outputs --
 *   rnb_mesh_loops_emit   with L, B, counts[8] and counts[9] as read: loop_offsets, loop_vertices, loop_status [L] uint8,
 *                         loop_edges [L] int32.  The place of a vertex in a SIMPLE loop comes from pointer jumping over the B
 *                         compacted boundary vertices, ceil(log2(longest SIMPLE loop)) rounds between two buffers; the other
 *                         loops' vertices from a stable radix split by loop id, one bit per pass.  No thread walks a loop.
 *   rnb_mesh_loops_mean   values [V,C] float64 (value_type 0) or float32 (1) -> means [L,C] of the same type, from the CSR
 *                         arrays alone (a vertex index outside [0, V) in loop_vertices is skipped, never used as an address).
 *   rnb_mesh_fill_emit    from the CSR arrays, loop_status and loop_centroid [L,3]: vertices_out [V + F,3], triangles_out
 *                         [T + N,3], filled [F] int32 (the loop of every new vertex), with F = counts[2] and N = counts[3] of a
 *                         count made with the same max_edges.
 * RNB_E_INVALID before any launch: a size out of range, V + F or T + N above 2^31 - 1, an unknown value_type.  RNB_E_NULL: a
 * required pointer (a workspace included) is NULL.  RNB_E_WORKSPACE: workspace_bytes below the query's answer.  Nothing is
 * allocated and no device-wide synchronisation happens inside these calls; every trip count is fixed before its loop. */
enum { RNB_LOOP_SIMPLE = 0, RNB_LOOP_TANGLED = 1, RNB_LOOP_MISORIENTED = 2 };
int rnb_mesh_fill_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes);
int rnb_mesh_loops_count(int64_t n_triangles, int64_t n_vertices, const void* topology_workspace,
                         size_t topology_workspace_bytes, const int32_t* boundary_labels, const int32_t* boundary_degree,
                         int64_t max_edges, void* workspace, size_t workspace_bytes, int64_t* counts, rnb_stream_t stream);
int rnb_mesh_loops_emit(int64_t n_triangles, int64_t n_vertices, const int32_t* boundary_labels, void* workspace,
                        size_t workspace_bytes, int64_t n_loops, int64_t n_boundary_vertices, int64_t longest_simple,
                        int64_t n_unwalked, int64_t* loop_offsets, int32_t* loop_vertices, uint8_t* loop_status,
                        int32_t* loop_edges, rnb_stream_t stream);
int rnb_mesh_loops_mean(const void* values, int32_t value_type, int64_t n_vertices, int64_t n_columns,
                        const int64_t* loop_offsets, const int32_t* loop_vertices, int64_t n_loops,
                        int64_t n_boundary_vertices, void* workspace, size_t workspace_bytes, void* means, rnb_stream_t stream);
int rnb_mesh_fill_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                       const int64_t* loop_offsets, const int32_t* loop_vertices, const uint8_t* loop_status,
                       const double* loop_centroid, int64_t n_loops, int64_t n_boundary_vertices, int64_t max_edges,
                       void* workspace, size_t workspace_bytes, int64_t n_filled, int64_t n_new_triangles,
                       double* vertices_out, int32_t* triangles_out, int32_t* filled, rnb_stream_t stream);

/* ---- Mesh evaluation: triangle bins, closest points on a mesh, area-weighted surface samples ----------------
 * What a reconstruction is judged by — how far is this mesh from that one (Chamfer, F-score) — needs two things for
 * many points at once: the exact nearest point ON a triangle mesh, and points spread evenly over a surface.  Both work
 * on the arrays of rnb_marching_cubes_emit / rnb_mesh_compact_emit in device memory:
 *   vertices [V,3] float64, triangles [T,3] int32, 0 <= V, T <= 2^31 - 1; queries [N,3] float64, N <= 2^31 - 1.
 * A triangle with a vertex index outside [0, V) or a non-finite coordinate is SKIPPED: never binned, never closest, area
 * 0, never sampled; every index is checked before it is used as an address.  Means, maxima and threshold counts over the
 * results are the caller's reductions: there is no reduction kernel, and no floating-point atomic anywhere.
 *
 * Bins.  rnb_mesh_bins is a uniform grid of cubic cells: cell (ix, iy, iz), linear index (iz * dims[1] + iy) * dims[0] + ix,
 * covers origin + [i, i + 1) * cell_size per axis; a coordinate maps to clamp(floor((x - origin) / cell_size), 0, dim - 1),
 * so the grid need not cover the mesh (what lies outside belongs to the boundary cells).  At most 2^24 cells.  A
 * triangle is entered into every cell its axis-aligned box overlaps.
 *   rnb_mesh_bins_count      cell_start [n_cells + 1] int64: the exclusive scan of the per-cell counts (the last element
 *                            is E); counts[0] = E, the number of entries; counts[1]: bit 0 (1) set when a triangle was
 *                            skipped, bit 1 (2) set when a binned triangle reaches outside the grid's box
 *                            origin + [0, dims] * cell_size (it is binned all the same) (device int64 [2]).
 *                            Workspace: rnb_mesh_bins_workspace_bytes(n_cells).
 *   -- the caller reads counts, decides whether the grid is too fine for this mesh, and allocates entries [E] --
 *   rnb_mesh_bins_emit       entries [E] int32 (the triangles of cell c are entries[cell_start[c] .. cell_start[c + 1]),
 *                            in an order that may differ from run to run: integer atomics on per-cell cursors) and
 *                            corners [T,9] float64, the three corners of every triangle side by side (zeros for a skipped
 *                            one), so that a query reads a triangle with one indirection.  Same grid, mesh and workspace
 *                            size as the count.
 *
 * Closest points.  rnb_mesh_closest_points: for every query the minimum over ALL binned triangles, under the
 * lexicographic order (dist2 as computed, triangle index), of the squared distance point-triangle:
 *     the minimum of |p - q|^2 over q = the closest point of each of the three edge SEGMENTS (parameter clamped to [0, 1];
 *     a zero-length edge is its end point) and, where the triangle has a normal and the projection of p onto its plane
 *     has barycentric weights >= 0, that projection — so a zero-area triangle is the segment or point it degenerates to.
 * Each pair's value is a pure function of its four points (tests/mesh_distance_ref.py is the same expression in numpy),
 * so the answer does not depend on the order of the entries or on the grid, and is bit-equal from run to run; the grid
 * only decides how many pairs are evaluated.  Search: Chebyshev shells of cells around the query's (clamped) cell,
 * stopped when everything outside the block searched so far is provably farther than the best so far
 * (csrc/mesh_eval.hip has the bound, valid for queries outside the box too, and the termination argument: every trip
 * count comes from the grid dims and E).  One lane per query: a caller who sorts the queries by cell makes neighbouring
 * lanes read the same entries.  flags: RNB_MESH_BINS_COVER states that bit 1 of counts[1] came back clear — no binned
 * triangle reaches outside the grid's box — which lets the bound count a query's distance to the box as well (fewer shells
 * for queries outside it, the same answers); it must not be set otherwise.
 *   dist2 [N] float64, closest [N,3] float64, triangle [N] int32: each may be NULL, not all.  A query with a non-finite
 *   coordinate: dist2 = NaN, closest = NaN, triangle = -1.  No binned triangle (E == 0): dist2 = +inf, closest = NaN,
 *   triangle = -1.  Nothing is launched for N == 0.
 *
 * Surface samples, area-weighted and deterministic (systematic sampling).
 *   rnb_mesh_sample_areas    cum_area [T] float64: C_t = inclusive sum of A_t = 0.5 |(b - a) x (c - a)| (0 for a skipped
 *                            triangle), in a fixed order: non-decreasing, C_t == C_{t-1} bit for bit where A_t == 0,
 *                            the same bits on every run; total [1] float64 (device) = A = C_{T-1} (0 for T == 0).  The
 *                            caller checks that A is positive and finite.  Workspace: rnb_mesh_sample_workspace_bytes(T).
 *   rnb_mesh_sample_surface  sample k of n:  u_k = ((k + xi) * A) / n, lowered to the largest double below A if it rounds up
 *                            to A; triangle t = the first with C_t > u_k (binary search, at most 32 steps): a triangle
 *                            of zero area is never chosen, and triangle t receives n A_t / A samples up to rounding.
 *                            The integer mixer, on unsigned 64-bit integers (the finaliser of splitmix64):
 *                                mix(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                                         z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *                                unit(z) = (z >> 11) * 2^-53
 *                                s = mix(seed);  xi = unit(s);  r1 = unit(mix(s ^ (2k)));  r2 = unit(mix(s ^ (2k + 1)))
 *                            (r1, r2) -> (1 - r1, 1 - r2) when r1 + r2 > 1 (decided exactly, as 1 - r1 < r2).
 *                            bary = (1 - r1 - r2, r1, r2): exact, >= 0, sum 1.  The point a + r1 (b - a) + r2 (c - a)
 *                            is evaluated as the convex combination (bary0 a + bary1 b) + bary2 c, each operation rounded
 *                            on its own.  points [n,3], bary [n,3], normal [n,3] float64 (the unit face normal
 *                            (b - a) x (c - a) / |.|; zero when undefined), triangle [n] int32: each may be NULL, not all.
 *                            If A is not positive and finite: triangle = -1 and zeros.  Nothing is launched for n == 0.
 * RNB_E_INVALID before any launch: a size negative or above 2^31 - 1, dims < 1 or more than 2^24 cells, cell_size or
 * origin not positive / finite, unknown flag bits, samples of a mesh without triangles.  RNB_E_NULL: a required pointer is NULL.
 * RNB_E_WORKSPACE: workspace_bytes below the query's answer.  Nothing is allocated and no device-wide synchronisation
 * happens inside these calls. */
enum { RNB_MESH_BINS_COVER = 1 };
typedef struct rnb_mesh_bins {
  double origin[3];
  double cell_size;   /* cubic cells */
  int32_t dims[3];
  int32_t reserved_;
} rnb_mesh_bins;
int rnb_mesh_bins_workspace_bytes(int64_t n_cells, int64_t* bytes);
int rnb_mesh_bins_count(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                        const rnb_mesh_bins* bins, void* workspace, size_t workspace_bytes, int64_t* cell_start,
                        int64_t* counts, rnb_stream_t stream);
int rnb_mesh_bins_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                       const rnb_mesh_bins* bins, void* workspace, size_t workspace_bytes, const int64_t* cell_start,
                       int64_t n_entries, int32_t* entries, double* corners, rnb_stream_t stream);
int rnb_mesh_closest_points(const double* queries, int64_t n_queries, const rnb_mesh_bins* bins, const int64_t* cell_start,
                            const int32_t* entries, int64_t n_entries, const double* corners, int64_t n_triangles,
                            int32_t flags, double* dist2, double* closest, int32_t* triangle, rnb_stream_t stream);
int rnb_mesh_sample_workspace_bytes(int64_t n_triangles, int64_t* bytes);
int rnb_mesh_sample_areas(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                          void* workspace, size_t workspace_bytes, double* cum_area, double* total, rnb_stream_t stream);
int rnb_mesh_sample_surface(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                            const double* cum_area, const double* total, int64_t n_samples, int64_t seed, double* points,
                            int32_t* triangle, double* bary, double* normal, rnb_stream_t stream);

/* ---- Mesh ray casting: the first hit of every ray with a binned mesh ------------------------------------------
 * What a camera sees of a mesh — depth, normal and silhouette per pixel, or whether a point is visible from an eye —
 * on the bins, entries and corners [T,9] of rnb_mesh_bins_count / rnb_mesh_bins_emit above (csrc/mesh_raycast.hip).
 *   origins, directions [N,3] float64; t_min, t_max [N] float64, each may be NULL (0 and +inf); N <= 2^31 - 1.
 * The hit point of a ray is o + t d with d AS GIVEN (not normalised).  rnb_mesh_raycast: for every ray the minimum over
 * ALL binned triangles, under the lexicographic order (t as computed, triangle index), over the triangles the ray hits
 * with t_min <= t <= t_max, both ends inclusive.  The pair test is the watertight one of Woop, Benthin and Wald
 * ("Watertight Ray/Triangle Intersection", JCGT 2013) in fp64, every operation rounded on its own:
 *     kz = argmax |d| (the first maximum); kx, ky = the next two axes cyclically, swapped when d[kz] < 0;
 *     Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz];
 *     per corner (A, then B and C alike), translated by -o:  Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz], Az = Sz * A[kz];
 *     U = Cx * By - Cy * Bx,  V = Ax * Cy - Ay * Cx,  W = Bx * Ay - By * Ax;
 *     a hit needs (U >= 0 && V >= 0 && W >= 0) || (U <= 0 && V <= 0 && W <= 0), then det = (U + V) + W != 0, then
 *     t = ((U * Az + V * Bz) + W * Cz) / det inside the range;  bary = (U, V, W) / det, the weights of (A, B, C).
 * ZERO COUNTS AS INSIDE (fp64 has no wider type to fall back on): a hit on an edge is reported by both neighbours and
 * the index order breaks the tie, so a closed surface has no pinholes.  A zero-area triangle has det == 0 and is never
 * hit: exactly so with two or three equal corners; with collinear, distinct corners det is zero up to rounding, and a
 * ray through the triangle's own segment (to within rounding) may be given a t inside the triangle's extent along the
 * ray.  Each pair's value is a pure function of the ray and the three corners (tests/mesh_raycast_ref.py is the same
 * expression in numpy), so the answer does not depend on the order of the entries and is bit-equal from run to run; it
 * does not depend on the grid either, the grid only deciding how many pairs are evaluated, FOR EVERY HIT WHOSE OWN POINT
 * sum of bary_k x corner_k LIES ON ITS RAY: within the widening below of o + t d.  That is every hit on a triangle with
 * |det| >= r^3 / (1024 S) (corners within r of the ray, S = the grid's magnitude + max |o|), i.e. not seen edge-on to
 * within its size over 1024 scene sizes.  A hit beyond that (the collinear triangle above is the extreme) is found by
 * a one-cell grid and may be missed by a finer one.  Search: one lane per ray, by layers of cells along
 * the major axis in the ray's direction, testing in each layer the cells under the ray's footprint widened by
 * 4096 x 2^-52 x (the grid's magnitude + max |o|), stopped at the first layer that starts behind the best t so far
 * (csrc/mesh_raycast.hip has the argument for why no hit is skipped, what it asks of a triangle seen edge-on, and why
 * every trip count comes from the grid dims and E).
 * flags MUST carry RNB_MESH_BINS_COVER (bit 1 of counts[1] came back clear: no binned triangle reaches outside the
 * grid's box): the walk visits only the cells under the ray, and a triangle outside the box sits in a boundary cell
 * far from where a ray meets it.  Without it the call is RNB_E_INVALID.
 *   t [N] float64, triangle [N] int32, bary [N,3] float64: each may be NULL, not all.  No hit: t = +inf, triangle = -1,
 *   bary = NaN.  A ray with a non-finite origin or direction, a zero direction or a NaN bound: t = NaN, triangle = -1,
 *   bary = NaN.  No binned triangle (E == 0): every ray misses.  Nothing is launched for N == 0.
 * RNB_E_INVALID before any launch: unknown flag bits, RNB_MESH_BINS_COVER missing, a size outside [0, 2^31 - 1], bins as
 * for the calls above.  RNB_E_NULL: a required pointer is NULL.  Nothing is allocated, no device-wide synchronisation. */
int rnb_mesh_raycast(const double* origins, const double* directions, const double* t_min, const double* t_max,
                     int64_t n_rays, const rnb_mesh_bins* bins, const int64_t* cell_start, const int32_t* entries,
                     int64_t n_entries, const double* corners, int64_t n_triangles, int32_t flags, double* t,
                     int32_t* triangle, double* bary, rnb_stream_t stream);

/* ---- Mesh culling by the cameras: per-(point, camera) status and per-point votes -----------------------------------
 * What the cameras of a masked multi-view reconstruction support of a mesh: for every point (a vertex) and every camera
 * whether the point projects into the frame, into the mask, and is not hidden by the mesh (csrc/mesh_cull.hip; one
 * launch for all cameras; tests/mesh_cull_ref.py is the same rule in numpy, and device and numpy agree bit for bit).
 *   points [N,3] float64; projections [C,3,4] float64 (P = K [R|t], world -> pixel, row-major); eyes [C,3] float64 (the
 *   camera centres); masks [C,H,W] uint8 (non-zero = inside) or NULL; the frame is H x W pixels either way; the bins,
 *   entries and corners of rnb_mesh_bins_count / rnb_mesh_bins_emit; N, C, E, T <= 2^31 - 1.
 * The status of the pair (camera c, point i = (X, Y, Z)), every operation in fp64 and rounded on its own:
 *   1. x = ((P00 X + P01 Y) + P02 Z) + P03, y and w alike from rows 1 and 2 of P_c.
 *      0 RNB_CULL_OUT_OF_FRAME if X, Y or Z is not finite, if w is not finite, or if w is not > 0.  Otherwise
 *      u = x / w, v = y / w, a = u + 0.5, b = v + 0.5, and status 0 unless 0 <= a < W and 0 <= b < H (tested in fp64,
 *      before any conversion to an integer; a NaN fails).  The pixel is (px, py) = (floor(a), floor(b)): pixel centres sit
 *      at integer coordinates, the convention of the ray generation, whose direction is Kinv (x, y, 1).
 *   2. 1 RNB_CULL_OUTSIDE_MASK if masks != NULL and masks[c, py, px] == 0.
 *   3. (skipped under RNB_CULL_NO_OCCLUSION: status 3.)  The segment o = eye_c, d = (X - ex, Y - ey, Z - ez), t_min = 0,
 *      t_max = 1 is cast by THE WALK AND PAIR TEST OF rnb_mesh_raycast (one device function serves both).  With t the
 *      first hit's parameter: 3 RNB_CULL_SEEN when t >= 1 - rel_tol (+inf, nothing met, counts), 2 RNB_CULL_OCCLUDED
 *      otherwise — a NaN t (a segment that cannot be cast: point == eye, an eye that is not finite) included.  That is
 *      what a cast of the segment through rnb_mesh_raycast followed by the same comparison answers, bit for bit.  With
 *      E == 0 every segment that can be cast is SEEN.
 *   counts [N,4] int32, ZEROED BY THE CALL: counts[i][k] = the number of cameras with status k, a row sums to C.
 *   status [C,N] uint8 or NULL.  Integer atomics only: bit-equal from run to run, whatever the launch geometry.
 * flags: RNB_MESH_BINS_COVER is required as for rnb_mesh_raycast; RNB_CULL_NO_OCCLUSION skips step 3 (eyes and the bins'
 * arrays may then be NULL).  Lanes of a wavefront are consecutive points of one camera.
 * RNB_E_INVALID before any launch: unknown flag bits, RNB_MESH_BINS_COVER missing, a size outside [0, 2^31 - 1], H or W
 * negative, or below 1 with masks given, rel_tol outside [0, 1), bins as for the calls above.  RNB_E_NULL: a required
 * pointer is NULL.  Nothing is launched for N == 0 or C == 0 (counts is zeroed for C == 0).  Nothing is allocated, no
 * device-wide synchronisation. */
enum { RNB_CULL_NO_OCCLUSION = 2 };   /* (shares the flag word with RNB_MESH_BINS_COVER = 1) */
enum { RNB_CULL_OUT_OF_FRAME = 0, RNB_CULL_OUTSIDE_MASK = 1, RNB_CULL_OCCLUDED = 2, RNB_CULL_SEEN = 3 };
int rnb_mesh_view_votes(const double* points, int64_t n_points, const double* projections, const double* eyes,
                        int64_t n_cameras, const uint8_t* masks, int32_t height, int32_t width, const rnb_mesh_bins* bins,
                        const int64_t* cell_start, const int32_t* entries, int64_t n_entries, const double* corners,
                        int64_t n_triangles, double rel_tol, int32_t flags, int32_t* counts, uint8_t* status,
                        rnb_stream_t stream);

/* ---- Texture baking: a per-triangle atlas, its lattice samples and the 8-bit images ----------------------------
 * What a simplified mesh loses between its vertices goes into textures (csrc/texture_bake.hip).  The atlas gives every
 * triangle a chart of the same size, so a texel's triangle follows from its coordinates by integer arithmetic alone; the
 * field is evaluated at the samples by rnb_mesh_vertex_attrs between the two calls below.  tests/texture_bake_ref.py is
 * this definition in numpy, and device and numpy agree bit for bit.
 *   vertices [V,3] float64 (model space), triangles [T,3] int32; V, T <= 2^31 - 1.
 * The atlas.  One parameter, the chart size s in [1, 255] (texel steps along a chart's legs); cell side c = s + 5.  Cell
 * k = t / 2 holds triangle 2k (its LOWER half) and 2k + 1 (its UPPER half); the K = ceil(T / 2) cells lie row-major,
 * `cols` per row, cell k with its top-left texel at ((k % cols) c, (k / cols) c) of a W x H image whose row 0 is the top
 * row (x runs right, y down).  Inside a cell, texel indices (i, j) in [0, c), a texel index standing for its centre:
 *                           lower half                       upper half
 *     vertex 0              (1, 1)                           (c - 2, c - 2)
 *     vertex 1              (1 + s, 1)                       (c - 2 - s, c - 2)
 *     vertex 2              (1, 1 + s)                       (c - 2, c - 2 - s)
 *     texels owned          i + j <= s + 3                   all others
 *     a1                    clamp(i - 1, 0, s)               clamp(c - 2 - i, 0, s)
 *     a2                    clamp(j - 1, 0, s - a1)          clamp(c - 2 - j, 0, s - a1)
 * (a1, a2) are the texel's lattice coordinates, a1, a2 >= 0, a1 + a2 <= s: a guard texel repeats a lattice sample of its
 * own triangle.  A texel is EMPTY when its triangle index is >= T (the upper half of the last cell for odd T, unused
 * cells), when it lies right of cols c or below the last cell row, or when its triangle is bad (below).  With c = s + 5 a
 * bilinear lookup at any point of a triangle's chart, edges and corners included, reads only texels that triangle owns
 * (with s + 4 the two hypotenuses would share a texel diagonal).  Corner UVs: u = (x + 0.5) / W, v = 1 - (y + 0.5) / H
 * with (x, y) the corner's texel in the image; both halves have the same, MIRRORED orientation in UV (vertex 0 -> 1 -> 2
 * turns clockwise in the (u, v) plane for both: (u1 - u0)(v2 - v0) - (v1 - v0)(u2 - u0) < 0).
 * Samples.  Triangle t has n_s = (s + 1)(s + 2) / 2 lattice samples, sample p = t n_s + r with
 *     r(a1, a2) = a2 (s + 1) - a2 (a2 - 1) / 2 + a1          (rows of constant a2; no compaction, no counting pass)
 * and the point, in fp64 with every quotient, product and sum rounded on its own, then converted to fp32:
 *     w1 = a1 / s,  w2 = a2 / s,  w0 = (s - a1 - a2) / s  (one division of an integer by s each; never 1 - w1 - w2)
 *     P = (w0 A + w1 B) + w2 C                             (A, B, C the corners 0, 1, 2)
 * So a corner sample equals its vertex converted to fp32, and a sample on a shared edge comes out the same from both
 * triangles (one weight is an exact zero, the other two are the same two quotients, a sum of two products commutes) — as
 * numbers (==); the sign of a zero coordinate is the only exception.  Seams need no blending pass.
 * A BAD triangle (an index outside [0, V), checked before use, or a non-finite corner) puts its samples at (0, 0, 0) and
 * its texels come out empty.
 *   rnb_texture_sample_points  points_out [count,3] float32 = the samples first .. first + count - 1 (a range may start
 *                              and end inside a triangle).  bad_out (may be NULL): int64 [1] on the device, ADDED to
 *                              (one integer add per wave): the bad triangles whose sample r = 0 lies in the range, so
 *                              ranges that partition [0, T n_s) count every bad triangle once; the caller zeroes it.
 *   rnb_texture_pack           one lane per texel.  rgb [T n_s,3] uint8 and normal [T n_s,3] float32: per-sample values
 *                              (each may be NULL with its image).  texel_sample [H,W] int32: the texel's sample index,
 *                              -1 where it is empty (the gather map for float channels).  albedo_image [H,W,4] uint8: the
 *                              sample's rgb with alpha 255, or 0,0,0,0.  normal_image [H,W,4] uint8: per component
 *                              rintf(255 (0.5 n + 0.5)) in fp32, every operation rounded on its own, clipped to
 *                              [0, 255] (NaN: 0), alpha 255 — object-space normals in model space; a zero normal gives
 *                              128; empty texels 0,0,0,0.  Each output may be NULL, not all; the images are written
 *                              one 32-bit word per texel and must be 4-byte aligned.  T == 0: the outputs are cleared
 *                              (images 0, texel_sample -1) without a kernel.
 * RNB_E_INVALID before any launch: s outside [1, 255]; a size negative or above 2^31 - 1; first + count > T n_s;
 * T n_s >= 2^31; W H >= 2^31; a layout whose cells do not hold T triangles inside W x H (cols c > W, or
 * cols (H / c) < K); every output NULL.  RNB_E_NULL: a required input is NULL.  Nothing is launched for T == 0 or
 * count == 0.  The one loop (the row of a rank) has s + 1 trips, fixed before it starts; no computed value becomes an
 * address unchecked.  Nothing is allocated, no device-wide synchronisation. */
typedef struct rnb_texture_layout {
  int32_t s;      /* chart size */
  int32_t cols;   /* cells per row */
  int32_t W, H;   /* image size in texels */
} rnb_texture_layout;
int rnb_texture_sample_points(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                              int32_t s, int64_t first, int64_t count, float* points_out, int64_t* bad_out,
                              rnb_stream_t stream);
int rnb_texture_pack(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                     const rnb_texture_layout* layout, const uint8_t* rgb, const float* normal, uint8_t* albedo_image,
                     uint8_t* normal_image, int32_t* texel_sample, rnb_stream_t stream);

/* The four rnb_gen_rays_* calls below that make rays are one kernel (csrc/raygen.hip) behind one set of checks: a front, the
 * pixel list of a train step (_at_view) or a range of a whole view's grid (_grid), and the targets, gathered from the finished
 * stacks or computed from the view's source maps (_from_maps).  The pixel-to-ray arithmetic exists once; it is unfused float32
 * with IEEE sqrt and division, the same bits whatever the front and the targets.
 *
 * Ray / target generation of one train_rnb step on the device: what Dataset.ps_gen_random_rays_at_view_on_all_lights
 * (models/dataset.py:351-376), the per-pixel light gather (exp_runner.py:214-220) and near_far_from_sphere
 * (models/dataset.py:448-458) compute on the host, for one view whose tensors are resident in device memory.
 *   intrinsics_inv, pose [4,4] row-major (intrinsics_all_inv[img_idx], pose_all[img_idx]);
 *   images, images_warmup, light_directions [n_lights, H, W, 3] of the view (each may be NULL with its output);
 *   mask [H, W, mask_channels] (channel 0 is used); pixels_x, pixels_y [B] int64, 0 <= x < W, 0 <= y < H.
 * Outputs: data [B,7] = rays_o | rays_v | mask; true_rgb, true_rgb_warmup, lights_dir [n_lights, B, 3];
 * near, far [B] (both or neither). */
int rnb_gen_rays_at_view(const float* intrinsics_inv, const float* pose, const float* images,
                         const float* images_warmup, const float* mask, int32_t mask_channels,
                         const float* light_directions, const int64_t* pixels_x, const int64_t* pixels_y, int64_t B,
                         int32_t n_lights, int32_t H, int32_t W, float* data, float* true_rgb,
                         float* true_rgb_warmup, float* lights_dir, float* near, float* far, rnb_stream_t stream);

/* Rays of a whole view (Dataset.gen_rays_at / gen_rays_between, models/dataset.py:300-326, :401-446) with the per-pixel
 * gathers of validate_image (exp_runner.py:409-410, :448), one launch: the rays [first, first + n) of the row-major
 * Hl x Wl grid whose pixel coordinates are tx [Wl] and ty [Hl] (device floats: torch.linspace(0, W - 1, W // l) made by
 * the caller, so the coordinates carry torch's bits).  intrinsics_inv / pose as rnb_gen_rays_at_view (pose may be an
 * interpolated one).  The optional sources mask [H,W,mask_channels], images, images_warmup, light_directions [n_lights,
 * H,W,3] are read at (rintf(ty), rintf(tx)): round-half-to-even, as torch.round.  `light`: one light index, or -1 for
 * all n_lights; Lo = 1 or n_lights.
 * Outputs: data [n,7] = rays_o | rays_v | mask (mask column 0 when mask is NULL); true_rgb, true_rgb_warmup, lights_dir
 * [Lo,n,3] (each NULL with or without its source); near, far [n] (both or neither). */
int rnb_gen_rays_grid(const float* intrinsics_inv, const float* pose, const float* tx, const float* ty, int32_t Wl,
                      int32_t Hl, int64_t first, int64_t n, const float* images, const float* images_warmup,
                      const float* mask, int32_t mask_channels, const float* light_directions, int32_t n_lights,
                      int32_t light, int32_t H, int32_t W, float* data, float* true_rgb, float* true_rgb_warmup,
                      float* lights_dir, float* near, float* far, rnb_stream_t stream);

/* Source mode of the two calls above: the same outputs computed per requested pixel from a view's normal, albedo and
 * mask maps (7 B per pixel as 8-bit images) instead of gathered from the finished stacks that Dataset.__init__ and
 * Dataset.gen_light_directions build on the host (models/dataset.py:100-298; 112 B per pixel).
 *   decode   integer elements: c = v / (float)M, M = 255 (U8) or 65535 (U16); normal n = 2c - 1 with its y and z
 *            components negated, albedo = c, mask = (c > 0.5) ? 1 : 0 (dataset.py:48-68, :134-136).  F32 normals and
 *            albedo are taken as already decoded (the reference's camera convention); an F32 mask is binarised (> 0.5).
 *   frame    a = n/|n|, negated when a_z < 0 (a = (0,0,1) for a zero normal).  b1, b2 = the branch-free basis of Duff
 *            et al., "Building an Orthonormal Basis, Revisited" (JCGT 2017) around a with sign = +1:
 *              q = -1 / (1 + a_z), r = a_x a_y q, b1 = (1 + a_x^2 q, r, -a_x), b2 = (r, 1 + a_y^2 q, -a_y);  b1 x b2 = a.
 *            This choice is part of the contract: lights_dir is a reproducible function of the pixel's normal.  The
 *            reference's frame has the same third axis and an arbitrary basis of the plane across it (what LAPACK's SVD
 *            returned for a repeated singular value), so its lights equal these up to a per-pixel rotation about a.
 *   lights   l_k = u_k.x b1 + u_k.y b2 + u_k.z a with u_k = local_lights[k];  lights_dir_k = view_pose[:3,:3] l_k
 *   colours  true_rgb_k = albedo max(n . l_k, 0);  true_rgb_warmup_k = albedo max(n . w_k, 0), w_k = warmup_lights_cam[k]
 *            (the raw n, not a; albedo = 1 when albedo is NULL: the reference's no_albedo).  A NaN normal gives NaN.
 * IEEE sqrt and division; rays, near / far and the data layout are those of the stack-mode calls, bit for bit. */
enum { RNB_SOURCE_U8 = 0, RNB_SOURCE_U16 = 1, RNB_SOURCE_F32 = 2 };
typedef struct rnb_source_maps {
  const void* normals;   /* [H,W,3] of normals_type */
  const void* albedo;    /* [H,W,3] of normals_type, or NULL (no_albedo) */
  const void* mask;      /* [H,W,mask_channels] of mask_type; channel 0 is used */
  int32_t normals_type;  /* RNB_SOURCE_*: element type of normals and albedo */
  int32_t mask_type;     /* RNB_SOURCE_* */
  int32_t H, W, mask_channels;
  int32_t n_lights;      /* 1 .. 8 (kMaxRenderLights) */
  float local_lights[8][3];      /* u_k: the main phase's lights in the per-pixel frame (b1, b2, a) */
  float warmup_lights_cam[8][3]; /* w_k: the warm-up phase's fixed camera-space lights */
} rnb_source_maps_t;
/* rnb_gen_rays_at_view on source maps.  pose is the view's own: it makes the rays and rotates the lights.
 * Outputs as rnb_gen_rays_at_view (true_rgb, true_rgb_warmup, lights_dir each optional; near, far both or neither).
 * RNB_E_NULL / RNB_E_INVALID before any launch: a NULL required pointer, an unknown type code, n_lights outside 1..8,
 * H, W, mask_channels or B below 1, near without far. */
int rnb_gen_rays_at_view_from_maps(const float* intrinsics_inv, const float* pose, const rnb_source_maps_t* source,
                                   const int64_t* pixels_x, const int64_t* pixels_y, int64_t B, float* data,
                                   float* true_rgb, float* true_rgb_warmup, float* lights_dir, float* near, float* far,
                                   rnb_stream_t stream);
/* rnb_gen_rays_grid on source maps, read at the rintf-rounded, clamped pixel.  pose makes the rays (it may be an
 * interpolated one); view_pose is the pose of the view the maps belong to and rotates its lights to world space.
 * Also refused before any launch: rays [first, first + n) outside the Hl x Wl grid, light outside -1 .. n_lights - 1. */
int rnb_gen_rays_grid_from_maps(const float* intrinsics_inv, const float* pose, const float* view_pose, const float* tx,
                                const float* ty, int32_t Wl, int32_t Hl, int64_t first, int64_t n,
                                const rnb_source_maps_t* source, int32_t light, float* data, float* true_rgb,
                                float* true_rgb_warmup, float* lights_dir, float* near, float* far, rnb_stream_t stream);

/* Camera adjoint of rnb_gen_rays_at_view / rnb_gen_rays_at_view_from_maps: d loss / d pose and d loss / d intrinsics_inv
 * from the adjoints of the rays, near / far and (source mode) the per-ray lights those calls produced, one launch.
 *   intrinsics_inv, pose [4,4]: the ones the forward used; pixels_x, pixels_y [B] int64: the forward's;
 *   lights_dir [n_lights,B,3]: the forward's output of the source-mode call (lights_dir = pose[:3,:3] l_cam), or NULL:
 *            stack-mode lights are gathered, not rotated, and have no camera adjoint;
 *   rays_o_bar, rays_d_bar [B,3], lights_bar [n_lights,B,3], near_bar, far_bar [B]: d loss / d output, each NULL = zero.
 * Per ray, recomputed from its pixel (x, y) in the forward's arithmetic:
 *   p = Kinv[:3,:3] (x, y, 1), n = |p|, v = p / n, d = R v, o = t, a = d.d, mid = -(o.d) / a  (near / far = mid -+ 1)
 *   m_bar = near_bar + far_bar;   o_bar += -m_bar d / a;   d_bar += -m_bar o / a + 2 m_bar (o.d) d / a^2
 *   pose_bar[:3,3]  = sum_b o_bar_b
 *   pose_bar[:3,:3] = sum_b d_bar_b v_b^T + sum_{l,b} lights_bar_{l,b} (R^T lights_dir_{l,b})^T
 *   v_bar = R^T d_bar;   p_bar = (v_bar - v (v.v_bar)) / n;   intrinsics_inv_bar[:3,:3] = sum_b p_bar_b (x, y, 1)^T
 * (R^T lights_dir recovers l_cam for an orthonormal R.)  Outputs: pose_bar [4,4]; intrinsics_inv_bar [4,4] or NULL (not
 * wanted); their last row, and intrinsics_inv_bar's last column, are written as 0: all 16 entries are defined.
 * The sums run in a fixed order without floating-point atomics (one workgroup: lane-local sums in ray order, a shuffle
 * butterfly, the waves in wave order), so the result's bits depend on the inputs only.  Gradients are those of the rays
 * given: under data parallelism they are shard-local like every other input gradient (no collective).
 * RNB_E_NULL / RNB_E_INVALID before any launch: a NULL required pointer (intrinsics_inv, pose, pixels, pose_bar),
 * lights_bar without lights_dir, B < 1, n_lights outside 0..8 (1..8 with lights_dir). */
int rnb_gen_rays_camera_bwd(const float* intrinsics_inv, const float* pose, const int64_t* pixels_x,
                            const int64_t* pixels_y, int64_t B, const float* lights_dir, int32_t n_lights,
                            const float* rays_o_bar, const float* rays_d_bar, const float* lights_bar,
                            const float* near_bar, const float* far_bar, float* pose_bar, float* intrinsics_inv_bar,
                            rnb_stream_t stream);

/* The loss of train_rnb (exp_runner.py:241-258) and its gradients with respect to the renderer outputs, one
 * launch:  loss = sum|(color_fine - true_rgb) * mask| / ((sum(mask) + 1e-5) * n_lights)
 *               + igr_weight * gradient_error
 *               + mask_weight * mean BCE(clip(weight_sum, 1e-3, 1 - 1e-3), mask),   mask := (mask > 0.5)
 * (mask := 1 when mask_weight == 0, exp_runner.py:233-236).  color_fine, true_rgb [n_lights, B, color_depth];
 * mask, weight_sum [B]; gradient_error [1].  loss [1]; parts [3] = color_loss, eikonal_loss, mask_loss;
 * d_color_fine / d_weight_sum / d_gradient_error = d loss / d input (same shapes as the inputs). */
int rnb_loss_rnb(const float* color_fine, const float* true_rgb, const float* mask, const float* weight_sum,
                 const float* gradient_error, int32_t n_lights, int64_t B, int32_t color_depth, float igr_weight,
                 float mask_weight, float* loss, float* parts, float* d_color_fine, float* d_weight_sum,
                 float* d_gradient_error, rnb_stream_t stream);
/* The same loss for one shard of a data-parallel batch, normalised by the GLOBAL batch (exp_runner.py:194
 * mask_sum and :251 BCE mean): batch_global [2] device floats = the all-reduced { sum of (mask > 0.5) (without the
 * 1e-5), number of rays } of the whole batch — the ray count is taken from the collective, not assumed to be
 * B * world, so unequal shards stay exact; gradient_error [1] = the GLOBAL eikonal ratio; eik_share = this shard's
 * share of it in the returned loss value (1/world).  loss/parts are this shard's ADDITIVE share: their sum over the
 * shards is the loss of the whole batch, and the sum over the shards of the gradients is its gradient.  (ABI 3: the
 * ray count moved from a host integer into batch_global[1].) */
int rnb_loss_rnb_shard(const float* color_fine, const float* true_rgb, const float* mask, const float* weight_sum,
                       const float* gradient_error, int32_t n_lights, int64_t B, int32_t color_depth, float igr_weight,
                       float mask_weight, const float* batch_global, float eik_share,
                       float* loss, float* parts, float* d_color_fine, float* d_weight_sum, float* d_gradient_error,
                       rnb_stream_t stream);

/* torch.optim.Adam.step() of exp_runner.py:115/:262 (amsgrad off) over ONE flat buffer of n parameters:
 * exp_avg / exp_avg_sq are the optimizer state, `step` the 1-based step count.  lr..weight_decay are host
 * scalars (the learning-rate schedule of exp_runner.py:327-337 changes lr every step). */
int rnb_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                  double beta1, double beta2, double eps, double weight_decay, int64_t step, rnb_stream_t stream);

/* Diagnostic (not part of the reference's interface): the largest magnitudes of one render's operands, read back from the
 * workspace of rnb_render_fwd (after it) and, for out[4], of rnb_render_bwd (after it) — same desc / B / S / flags / ws as those
 * calls.  out: device [8] floats:
 *   [0] max |effective weight| over the matrices of both networks (0 unless the default x2h arithmetic keeps its scale table)
 *   [1] max |hidden activation or encoded input| of the SDF network      [2] max |Jacobian row| of the normal's reverse sweep
 *   [3] max |input or hidden activation| of the albedo network           [4] max |loss adjoint| recorded by the backward (x2h)
 *   [5] after rnb_render_bwd: the number of 64-point tiles the fused albedo backward skipped because their colour adjoint was
 *       exactly zero (0 where that path is off: RNB_VARIANT_NO_DEAD_TILES, other routes)
 *   [6..7] 0 (reserved).
 * The default arithmetic (RNB_VARIANT_X2H) takes every fp16 operand scale from the data — per matrix, per tile and layer, per
 * launch — so none of these has a limit; the numbers document how far a model is from the fixed scales' old range (255 /
 * 1023), e.g. over a training run (tools/soak.py, profiles/r05_x2h_range.txt).  Costs one pass over the saved state: not
 * for the hot path.  [ABI 5] */
int rnb_render_range(const rnb_model_desc* desc, const float* packed, const void* ws, size_t ws_bytes, int64_t B, int32_t S,
                     int32_t flags, float* out, rnb_stream_t stream);

/* Measurement aid for bench.py (not part of the reference's interface): while enabled, every launch of
 * the fp32-MFMA kernels (fused_*_kernel, gemm_dw_*_kernel, gemm_rows_kernel<...>) is bracketed by HIP events on
 * its launch stream.  After the caller has synchronised, rnb_profile_collect returns the summed device
 * time (ms), the number of launches and their summed algorithmic FLOPs (real layer shapes) since the
 * last enable/collect.  This is the only mutable global state of the library; it is off by default. */
int rnb_profile_enable(int on);
int rnb_profile_collect(double* gemm_ms, int64_t* gemm_launches, double* gemm_flops);
/* Per kernel class of the last rnb_profile_collect: one text line "<class> <ms> <launches> <flops>" each, written to
 * `out` (NUL-terminated, at most `capacity` bytes; out may be NULL); returns the number of bytes the full text needs. */
int64_t rnb_profile_report(char* out, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* RNBNEUS_H */
