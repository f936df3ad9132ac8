/*
 * vfn.h — C ABI of the MI355X-native VF-NeRF volume-rendering hot path.
 *
 * This is the drop-in boundary: every entry point is stateless and stream-ordered, takes plain
 * DEVICE pointers + sizes + a POD parameter struct + the hipStream_t to launch on (passed as
 * void*), allocates nothing, and returns 0 on success or a negative vfn_status (message via
 * vfn_last_error()).  All tensors are dense row-major fp32 unless stated.  The reference is pure
 * Python, so there is no pre-existing FFI; each entry names the reference function it replaces
 * (paths relative to the reference root) and INTEGRATION.md shows the ctypes binding the facade uses.
 *
 * Notation: N rays, S_c coarse samples, N_f fine samples, S_t = S_c + N_f, M points.
 */
#ifndef VFN_H
#define VFN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a POD struct's layout or an entry point's signature changes (2: vfn_render_params.timing_events,
 * vfn_abi_struct_bytes; 3: vfn_f16x3_set_clock_probe, vfn_train_step, vfn_linear_rows_dx_sums; 4: the session form of vfn_train_step —
 * VFN_TRAIN_RENDER / VFN_TRAIN_BACKWARD, vfn_train_step_workspace_layout, vfn_train_step_supervision_points / _forward / _backward; 5: vfn_select_samples,
 * the training selection of vfn_train_step's sparse colour branch, vfn_grid_lattice_points, vfn_linear_rows_fold, vfn_weight_grad_partials_bf16_fold).  The Python binding reads this constant from this file and refuses a library
 * that reports another. */
#define VFN_ABI_VERSION 5

typedef enum vfn_status {
    VFN_OK = 0,
    VFN_ERR_INVALID = -1,     /* bad argument / unsupported shape */
    VFN_ERR_LAUNCH = -2,      /* HIP launch error */
    VFN_ERR_UNSUPPORTED = -3  /* network geometry the kernels are not specialised for */
} vfn_status;

/* Thread-local message of the last failing call on this thread ("" if none). */
const char* vfn_last_error(void);
int vfn_abi_version(void);
/* sizeof() of the POD structs of this header as the library was compiled, by index: 0 vfn_net_geom, 1 vfn_layer_params,
 * 2 vfn_raygen_params, 3 vfn_density_params, 4 vfn_fine_params, 5 vfn_render_params, 6 vfn_unfold_entry, 7 vfn_wgrad_layer,
 * 8 vfn_loss_params, 9 vfn_train_step_params, 10 vfn_train_step_io;
 * -1 for any other index.  A binding checks its own mirrors of the structs against these (tests/test_host_logic.py). */
int32_t vfn_abi_struct_bytes(int32_t which);

/* ---------------------------------------------------------------------------------------------
 * Network geometry + packed weights.
 *
 * The kernels are specialised for the shipped architecture family (confs/vf_nerf.conf:13-37):
 * hidden width 256 everywhere, ReLU between layers, eval-mode BatchNorm folded into each Linear,
 * one optional skip layer that concatenates the positional encoding (vector_field_network.py:192-193),
 * VF head = 3 vector columns + F feature columns with tanh, rendering head = 3 columns with sigmoid.
 * ------------------------------------------------------------------------------------------- */
#define VFN_MAX_LAYERS 16
#define VFN_HIDDEN 256

typedef struct vfn_net_geom {
    int32_t n_layers;        /* number of Linear layers (VF: 9, render: 5 in the shipped conf)          */
    int32_t multires;        /* positional-encoding octaves L (embedder.py:40-52); VF: 6, render: 4     */
    int32_t skip_layer;      /* index of the layer whose input is cat([x, PE])/sqrt(2); -1 = none       */
    int32_t feature_dims;    /* VF: F (256 or 0); render: width of the feature input (256 or 0)         */
    int32_t in_dims[VFN_MAX_LAYERS];   /* reference in_features of each Linear                          */
    int32_t out_dims[VFN_MAX_LAYERS];  /* reference out_features of each Linear                         */
    int32_t has_bn[VFN_MAX_LAYERS];    /* 1 when the Linear is followed by BatchNorm1d                  */
} vfn_net_geom;

/* Raw (reference-layout) parameter pointers of one layer: Linear weight[out][in], bias[out], and the
 * BatchNorm1d weight/bias/running_mean/running_var[out] (NULL when has_bn == 0). */
typedef struct vfn_layer_params {
    const float* weight;
    const float* bias;
    const float* bn_weight;
    const float* bn_bias;
    const float* bn_mean;
    const float* bn_var;
} vfn_layer_params;

#define VFN_NET_VF 0
#define VFN_NET_RENDER 1

/* Number of floats of the packed-weight workspace for a network of this geometry (host-side, no GPU).
 * Returns < 0 (vfn_status) when the geometry is unsupported. */
int64_t vfn_packed_size(int32_t net_kind, const vfn_net_geom* geom);

/* Fold eval-mode BatchNorm (eps 1e-5) and the skip 1/sqrt(2) into each Linear and re-order the result
 * into the MFMA-fragment order the fused kernels stream (see DESIGN.md "packed weights").  Must be
 * re-run after every optimizer step; reads the live parameter storage, writes `packed`.
 * Replaces: the per-call nn.Linear/nn.BatchNorm1d parameter reads of vector_field_network.py:177-208
 * and rendering_network.py:98-103. */
int vfn_pack_weights(int32_t net_kind, const vfn_net_geom* geom, const vfn_layer_params* layers,
                     float* packed, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K1 — rays + coarse sampler.
 * Replaces utils/rendering.py:12-60 (+ utils/pinhole_model.py:9-63) and
 * models/samplers/ray_sampler.py:49-80,113-142.
 * ------------------------------------------------------------------------------------------- */
typedef struct vfn_raygen_params {
    int32_t n_rays;
    int32_t n_samples;       /* S_c */
    int32_t pose_is_quat;    /* 0: pose[N,4,4]; 1: pose[N,7] = (qr,qi,qj,qk,tx,ty,tz) */
    float near;
    float far;               /* used when far_per_ray == NULL */
} vfn_raygen_params;

/* uv[N,2] (u = x, v = y), pose, intrinsics[N,4,4], t_vals[S_c] = linspace(0,1,S_c) (host supplied so
 * that it is bit-identical to torch.linspace), far_per_ray[N] or NULL, u_coarse[N,S_c] uniforms in
 * [0,1) or NULL for deterministic sampling.
 * Outputs: directions[N,3] (un-normalised, Q7), ray_dirs[N,3] (unit), cam_loc[N,3], z_vals[N,S_c],
 * points[N,S_c,3]. */
int vfn_raygen_uniform(const vfn_raygen_params* p, const float* uv, const float* pose, const float* intrinsics,
                       const float* t_vals, const float* far_per_ray, const float* u_coarse,
                       float* directions, float* ray_dirs, float* cam_loc, float* z_vals, float* points,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2/K4 — fused MLPs (fp32 MFMA, weights from vfn_pack_weights).
 * ------------------------------------------------------------------------------------------- */
/* points[M,3] -> out.  out_cols == 3: only the vector columns [M,3] (proposal pass, grid queries:
 * vector_field_nerf.py:253-256, evaluation/utils/mc_utils.py:100); out_cols == 3+F: the full
 * [M,3+F] row (vector_field_network.py:140-208, eval mode). */
int vfn_vf_mlp_fwd(const vfn_net_geom* geom, const float* packed, const float* points, int64_t n_points,
                   int32_t out_cols, float* out, void* stream);

/* Rendering MLP alone: rendering_network.py:62-108 (mode "idr").  view_dirs[M,3] per point. */
int vfn_render_mlp_fwd(const vfn_net_geom* geom, const float* packed, const float* points, const float* normals,
                       const float* view_dirs, const float* feats, int64_t n_points, float* colors,
                       void* stream);

/* Fine pass in one launch: VF MLP -> (features stay in LDS) -> rendering MLP.
 * points[M,3] with M = N*S_t, ray_dirs[N,3]; row m uses ray_dirs[m / samples_per_ray].
 * Outputs normals[M,3] (tanh'ed vector columns) and colors[M,3] (sigmoid); feats_out[M,F] optional
 * (NULL to skip).  Replaces vector_field_nerf.py:294-297 + :315-318. */
int vfn_vf_render_fused_fwd(const vfn_net_geom* vf_geom, const float* vf_packed,
                            const vfn_net_geom* rn_geom, const float* rn_packed,
                            const float* points, const float* ray_dirs, int64_t n_points,
                            int32_t samples_per_ray, float* normals, float* colors, float* feats_out,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * K3 — per-ray density -> VolSDF weights (-> argmax / composite).
 * Replaces vector_field_nerf.py:442-474 (get_density), models/helpers/functions.py:41-72,
 * models/helpers/density_functions.py:129-204, utils/rendering.py:122-148 and the sums at
 * vector_field_nerf.py:322-323.
 * ------------------------------------------------------------------------------------------- */
typedef struct vfn_density_params {
    int32_t n_rays;
    int32_t n_samples;        /* S: samples per ray in this pass                                   */
    int32_t n_window;         /* W = len(cos_sim_weights); uniform ones/W weights are used (Q6)     */
    int32_t normalize;        /* normalize_rendering                                                */
    float dir_to_normal_th;
    float beta_min, beta_max; /* density_config.beta_bounds                                         */
    float mean_min, mean_max; /* density_config.mean_bounds                                         */
    float scale_min;
    float cutoff;             /* -0.5: the reference drops the configured cutoff (Q5)               */
} vfn_density_params;

/* normals[N,S,3], ray_dirs[N,3], z_vals[N,S]; density_scalars = device pointer to {beta, mean, scale}
 * (raw, un-clamped learnable values).  Outputs (any may be NULL): sigma[N,S], weights[N,S],
 * argmax[N] int64 (first maximum of weights), and, when colors[N,S,3] is given, rgb[N,3] and
 * depth[N] (= sum_s w c, sum_s w z). */
int vfn_ray_density_weights(const vfn_density_params* p, const float* normals, const float* ray_dirs,
                            const float* z_vals, const float* density_scalars, const float* colors,
                            float* sigma, float* weights, int64_t* argmax, float* rgb, float* depth,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * K3b — range fine sampler.  Replaces models/samplers/ray_sampler.py:264-302 + :77-78.
 * ------------------------------------------------------------------------------------------- */
typedef struct vfn_fine_params {
    int32_t n_rays;
    int32_t n_coarse;   /* S_c */
    int32_t n_fine;     /* N_f = min(N_samples, max_samples) */
    float near;
    float far;          /* used when far_per_ray == NULL */
    float half_range;   /* fine_range, as fp32 */
    float window_step;  /* fp32(2*fine_range/(N_f-1)) evaluated in double by the host, as Python does */
    float span;         /* fp32(far - near) evaluated in double by the host; ignored with far_per_ray */
} vfn_fine_params;

/* z_coarse[N,S_c], argmax[N] (from vfn_ray_density_weights), directions[N,3], cam_loc[N,3],
 * u_fine[N,N_f] or NULL (deterministic window), u_add[N,N_f] (always consumed, Q9).
 * Outputs z_vals[N,S_t] ascending, points[N,S_t,3]. */
int vfn_range_fine_sample(const vfn_fine_params* p, const float* z_coarse, const int64_t* argmax,
                          const float* directions, const float* cam_loc, const float* far_per_ray,
                          const float* u_fine, const float* u_add, float* z_vals, float* points, void* stream);

/* The same sampler, additionally reporting the provenance of every sorted sample, so that a caller that already holds
 * per-sample results for the proposal samples (the reference evaluates the vector-field net on them twice:
 * vector_field_nerf.py:252-277 and :294-297) can evaluate only the N_f new ones and gather:
 * src[N,S_t] = ray*S_c + j for proposal sample j of the ray, new_row0 + ray*N_f + k for new sample k (new_row0 >= N*S_c:
 * the row at which the caller stores the new samples' results); new_points[N,N_f,3] are the new samples in generation
 * order; dst[new_row0 + N*N_f] is the inverse map, dst[src[i]] = i (rows no sample comes from are left untouched).
 * Each of the three may be NULL. */
int vfn_range_fine_sample_indexed(const vfn_fine_params* p, const float* z_coarse, const int64_t* argmax,
                                  const float* directions, const float* cam_loc, const float* far_per_ray,
                                  const float* u_fine, const float* u_add, float* z_vals, float* points, int32_t* src,
                                  float* new_points, int32_t* dst, int64_t new_row0, void* stream);

/* The samplers as stand-alone calls, for callers that sample through the sampler OBJECTS rather than through render():
 * UniformSampler.get_z_vals / RaySampler.sample (models/samplers/ray_sampler.py:113-142, :49-80) on given
 * directions[N,3] (un-normalised, Q7) / cam_loc[N,3]: z = near (1 - t) + far t, stratified with u[N,S] when given
 * (NULL = deterministic), points = cam_loc + z * directions (points may be NULL: depths only).  Same arithmetic, in the
 * same order, as vfn_raygen_uniform: bit-identical depths. */
int vfn_uniform_sample(int32_t n_rays, int32_t n_samples, float near, float far, const float* directions,
                       const float* cam_loc, const float* t_vals, const float* far_per_ray, const float* u,
                       float* z_vals, float* points, void* stream);

/* out[r] = index of the FIRST maximum of row r of w[n_rows, n_cols] (torch.argmax(coarse_weights, dim=-1),
 * ray_sampler.py:277; an all-zero row gives 0, Q9), int64. */
int vfn_rows_argmax(const float* w, int32_t n_rows, int32_t n_cols, int64_t* out, void* stream);

/* The sample selection of the sparse colour branch (vfn_render_fwd with sparse_colours, vfn_train_step with sparse_colours) on its own:
 * weights[N,S], points[N,S,3], ray_dirs[N,3] -> count[0] = K (device memory), and for k < K in ray order: index[k] = ray * S + j,
 * points_sel[k], dirs_sel[k] (each sized for N * S rows).  sigma == z_vals == NULL: the samples with w > 0 — all a forward render's
 * rgb = sum w c needs (models/nerf/vector_field_nerf.py:322).  With sigma[N,S] and z_vals[N,S]: additionally the samples whose weight is
 * zero by an underflowed alpha alone (sigma > 0, delta > 0, T > 0: d w / d sigma = T delta exp(-sigma delta) is not zero there, and the
 * backward of utils/rendering.py:122-148 multiplies it with the sample's colour) — the selection a training step uses.
 * scratch: 2 N int32. */
int vfn_select_samples(const float* weights, const float* sigma, const float* z_vals, int32_t n_rays, int32_t n_samples, const float* points,
                       const float* ray_dirs, int32_t* scratch, int32_t* count, int32_t* index, float* points_sel, float* dirs_sel, void* stream);

/* RaySampler.sample with additional_depths (ray_sampler.py:69-73): z_out[N, S + E] = sort(cat(z_vals[N,S], extra[N,E])) per ray
 * (ascending, NaN last, like torch.sort), points[N, S + E, 3] = cam_loc + z_out * directions (NULL: depths only).  S + E <= 2048. */
int vfn_merge_sort_depths(const float* z_vals, const float* extra, int32_t n_rays, int32_t n_samples, int32_t n_extra,
                          const float* directions, const float* cam_loc, float* z_out, float* points, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The whole gradient-free render() in ONE call: VectorFieldNerf.render (models/nerf/vector_field_nerf.py:216-338) on the f16x3
 * kernels with one vector-field evaluation per distinct sample, issued from C on one stream out of one caller-supplied workspace
 * (vfn_render_fwd_workspace_bytes; no allocation, no synchronisation) as FIVE launches: rays + proposal samples (missing draws
 * generated in place) | fused VF + rendering net on the proposal samples | proposal weights -> argmax -> range fine sampler |
 * the fused launch on the new samples, outputs scattered | weights + composite (which also moves the proposal samples' normals
 * and colours to their sorted positions).  The per-ray launches run the kernels of vfn_raygen_uniform, vfn_fill_uniform,
 * vfn_ray_density_weights, vfn_range_fine_sample_indexed and vfn_scatter_rows3, so every value equals what those entry points
 * produce called one by one.
 * Random draws: u_coarse[N,S_c] / u_fine[N,N_f] (read only when the matching perturb flag is set) and u_add[N,N_f] (always
 * consumed, Q9) may each be NULL, in which case they come from the Philox stream (seed, offset) in that order; the call
 * consumes ceil(generated / 4) counter values.  far_*_per_ray: optional [N] (ray_sampler.py:126-127).
 * Outputs: ray_dirs[N,3] (unit), z_vals[N,S_t], points[N,S_t,3], normals[N*S_t,3], colors[N*S_t,3], weights[N,S_t], rgb[N,3],
 * depth[N]; N*S_t < 2^22. */
typedef struct vfn_render_params {
    int32_t n_rays, n_coarse, n_fine;   /* N, S_c, N_f = min(fine_sampler.N_samples, max_samples) */
    int32_t pose_is_quat;
    int32_t perturb_coarse, perturb_fine;
    float near_coarse, near_fine;       /* ray_sampler.near, fine_sampler.near (the trainer sets both from the dataset bounds) */
    float far_coarse, far_fine;         /* used when the per-ray pointer is NULL */
    float fine_range, window_step, span; /* as in vfn_fine_params: window_step, span evaluated in double by the host */
    vfn_density_params density;         /* n_rays / n_samples are filled in per pass */
    uint64_t seed, offset;              /* Philox stream for the draws not supplied */
    int32_t colour_products;            /* 0 or 3: three products everywhere; 2: the colour branch on two (vfn_vf_render_fused16_products) */
    int32_t separate_launches;          /* 0: the five merged launches; 1: the same pipeline through the stand-alone entry points (eight) */
    int32_t streams;                    /* 2: the batch in two halves, the second on an internal side stream forked from and joined
                                         * into `stream` (same values; the halves fill each other's partial rounds); 1: one stream;
                                         * 0: two halves when the fused launches would leave >= 5 % of their workgroup slots empty */
    int32_t sparse_colours;             /* != 0 (opt-in): colours are evaluated only for the samples whose weight is non-zero — the vector-field
                                         * net on every sample with its vector-only launch, the fused VF + rendering launch on the compacted list
                                         * of samples with w > 0 (a count the host never learns).  rgb, depth, weights, normals, z_vals, points are
                                         * bit-identical to the dense plan; `colors` holds zeros where w = 0.  For callers that keep rgb / depth
                                         * only (evaluation/methods.py:528-540) */
    void* timing_events[4];             /* optional hipEvent_t handles (NULL: none), recorded on the launch stream around the two fused
                                         * VF + rendering launches: [0] before / [1] after the one on the proposal samples, [2] / [3] the one
                                         * on the new samples (with `streams` > 1: around the FIRST range's launches).  bench.py times the
                                         * dominant kernel with these without leaving the one-call path. */
    uint32_t* status_word;              /* optional (ABI 4): where the f16x3 launches of THIS call report operands outside their range (bit 0:
                                         * a hidden activation reached the f16 clamp, bit 1: an input coordinate did) — per call, no hidden
                                         * state; NULL: wherever vfn_f16x3_set_status (the ABI-3 setter, kept as a shim) pointed this thread */
    uint64_t* clock_stamps;             /* optional (ABI 4): [clock_slots][2] per-workgroup (shader-clock cycles, 100 MHz ticks) of the fused
                                         * launches of THIS call (vfn_f16x3_set_clock_probe is the ABI-3 shim) */
    int64_t clock_slots;
} vfn_render_params;
int64_t vfn_render_fwd_workspace_bytes(const vfn_render_params* p);
int vfn_render_fwd(const vfn_render_params* p, const vfn_net_geom* vf_geom, const void* vf_packed16,
                   const vfn_net_geom* rn_geom, const void* rn_packed16, const float* uv, const float* pose,
                   const float* intrinsics, const float* t_vals, const float* far_coarse_per_ray,
                   const float* far_fine_per_ray, const float* density_scalars, const float* u_coarse,
                   const float* u_fine, const float* u_add, void* workspace, float* ray_dirs, float* z_vals,
                   float* points, float* normals, float* colors, float* weights, float* rgb, float* depth,
                   void* stream);

/* Counter-based uniforms in [0,1) for production sampling (Philox4x32-10, one 4-tuple per 4 outputs). */
int vfn_fill_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* =============================================================================================
 * Training path (autograd of the fine pass: models/nerf/vector_field_nerf.py:294-323 under
 * train/vector_field_nerf_train.py:251-260, eval-mode BatchNorm as in :140-141).
 *
 * Workspace layout shared by the entry points below ("slots"): slot s is a dense [M,256] fp32 matrix;
 * slots 0..H_vf-1 are the VF net's hidden layers in order (the last one is the 256-wide feature block of
 * the final Linear when feature_dims > 0), slots H_vf..H_vf+H_rn-1 the rendering net's hidden layers.
 * `saved` holds post-activation outputs (forward), `dy` pre-activation gradients (backward).
 * ============================================================================================= */

/* Size (floats) and fill of the TRANSPOSED weight pack used by dX = dY * W'. */
int64_t vfn_packed_bwd_size(int32_t net_kind, const vfn_net_geom* geom);
int vfn_pack_weights_bwd(int32_t net_kind, const vfn_net_geom* geom, const vfn_layer_params* layers,
                         float* packed_bwd, void* stream);

/* Forward kernels that additionally write `saved` slots and the auxiliary input tiles
 * (save_aux_vf[M,40] = positional encoding of the point, save_aux_rn[M,40] = [p, PE(d), n]). */
int vfn_vf_mlp_fwd_train(const vfn_net_geom* geom, const float* packed, const float* points, int64_t n_points,
                         int32_t out_cols, float* out, float* saved, float* save_aux_vf, void* stream);
int vfn_vf_render_fused_fwd_train(const vfn_net_geom* vf_geom, const float* vf_packed,
                                  const vfn_net_geom* rn_geom, const float* rn_packed,
                                  const float* points, const float* ray_dirs, int64_t n_points,
                                  int32_t samples_per_ray, float* normals, float* colors, float* saved,
                                  float* save_aux_vf, float* save_aux_rn, void* stream);

/* dX chain.  rn_geom != NULL: gradients d_colors[M,3] (wrt the sigmoid outputs `colors`) and d_vec (wrt the
 * tanh'ed vector columns `vec`, row stride vec_stride) are pushed back through the rendering net, the feature
 * hand-off and the VF net.  rn_geom == NULL: VF net only; d_feats (wrt the tanh'ed features, row stride
 * vec_stride) may be NULL.  Writes every `dy` slot plus dz_rgb[M,4] / dz_vec[M,4] (pre-activation gradients of
 * the two 3-channel heads, 4th column zero). */
int vfn_mlp_bwd_chain(const vfn_net_geom* vf_geom, const float* vf_packed, const float* vf_packed_bwd,
                      const vfn_net_geom* rn_geom, const float* rn_packed, const float* rn_packed_bwd,
                      const float* saved, float* dy, const float* d_colors, const float* colors,
                      const float* d_vec, const float* vec, const float* d_feats, int32_t vec_stride,
                      int64_t n_points, float* dz_rgb, float* dz_vec, void* stream);

/* Weight-gradient partials dW'[n][k] = sum_m dY[m][n] X[m][k] as `groups` slabs [groups][n_out][ld_out], plus
 * db'[n] = sum_m dY[m][n] as [groups][n_out] (db_part may be NULL).  shape 0: n_out 256, ld_out 256 (hidden
 * layer, act inputs); 1: n_out 256, ld_out 64 (aux inputs); 2: n_out 32, ld_out 256 (3-channel head).
 * Columns >= n_valid of dY / >= k_valid of X read as zero. */
int vfn_weight_grad_partials(int32_t shape, const float* dy, int32_t ld_dy, int32_t n_valid, const float* x,
                             int32_t ld_x, int32_t k_valid, int64_t n_points, int32_t groups, float* dw_part,
                             float* db_part, int32_t x_f16, void* stream);
/* x_f16 != 0 (shape 2 only): the rows of X hold 256 f16 values in their first 512 bytes (the opt-in storage of the f16x3
 * training forwards, see vfn_vf_mlp16_fwd_train); likewise for vfn_weight_grad_partials_bf16. */

/* Backward of vfn_ray_density_weights: upstream d_rgb[N,3], d_depth[N], d_weights[N,S] (each may be NULL) ->
 * d_colors[N,S,3] (written, may be NULL), d_normals[N,S,3] (ACCUMULATED into), d_scalars[3] (atomically
 * accumulated gradients of the raw beta, mean, scale).  n_samples <= 256. */
int vfn_ray_density_weights_bwd(const vfn_density_params* p, const float* normals, const float* ray_dirs,
                                const float* z_vals, const float* density_scalars, const float* colors,
                                const float* d_rgb, const float* d_depth, const float* d_weights,
                                float* d_normals, float* d_colors, float* d_scalars, void* stream);

/* Backward of the density alone — VectorFieldNerf.get_density under autograd (models/nerf/vector_field_nerf.py:442-474 is
 * part of the reference's graph): upstream d_sigma[N,S] -> d_normals[N,S,3] (ACCUMULATED into), d_scalars[3]
 * (atomically accumulated, may be NULL).  z_vals[N,S] only feeds the composite terms, which carry no gradient here. */
int vfn_ray_density_sigma_bwd(const vfn_density_params* p, const float* normals, const float* ray_dirs,
                              const float* z_vals, const float* density_scalars, const float* d_sigma,
                              float* d_normals, float* d_scalars, void* stream);

/* =============================================================================================
 * "f16x3" inference kernels: the same MLPs on the f16 matrix cores with fp32-equivalent accuracy.
 * Every value is carried as two halves (hi + lo, 22 significant bits) and each product is evaluated as
 * a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation: 3 f16 MFMAs per K=16
 * block instead of 8 fp32 MFMAs.  Weights come from vfn_pack16_weights (BatchNorm folded, scaled by 2^6, split,
 * fragment order; re-run after every optimizer step).  Specialised for the shipped layer shapes
 * (confs/vf_nerf.conf:13-37); other geometries return VFN_ERR_UNSUPPORTED and callers use the fp32 kernels.
 * ============================================================================================= */
int64_t vfn_pack16_size(int32_t net_kind, const vfn_net_geom* geom);           /* bytes */
int vfn_pack16_weights(int32_t net_kind, const vfn_net_geom* geom, const vfn_layer_params* layers,
                       void* packed16, void* stream);
/* points[M,3] -> the 3 tanh'ed vector columns [M,3] (proposal pass / grid queries). */
int vfn_vf_mlp16_fwd(const vfn_net_geom* geom, const void* packed16, const float* points, int64_t n_points,
                     float* out_vec, void* stream);
/* Fine pass: VF MLP -> rendering MLP, features stay in registers; normals[M,3], colors[M,3]. */
int vfn_vf_render_fused16_fwd(const vfn_net_geom* vf_geom, const void* vf_packed16, const vfn_net_geom* rn_geom,
                              const void* rn_packed16, const float* points, const float* ray_dirs,
                              int64_t n_points, int32_t samples_per_ray, float* normals, float* colors,
                              void* stream);

/* Range guard of the f16x3 kernels.  The split representation covers |activation| < ~937 (the ReLU epilogue clamps the 2^6-scaled
 * value at 60 000 so that an out-of-family value degrades instead of becoming inf - inf), |input coordinate| likewise, and
 * folded weights whose largest entry per layer is neither in the f16 denormal range nor beyond 65 504.  The reference has no
 * such restriction (vector_field_network.py:177-208), so the kernels REPORT when they leave it:
 *  - vfn_f16x3_set_status(word): every later f16x3 launch of the calling thread ORs into *word (device memory, 4 bytes) bit 0
 *    when a hidden activation hit the clamp and bit 1 when an input did; NULL switches the reporting off.  Thread-local.
 *  - vfn_pack16_weights writes, behind the pack (the last 256 bytes of the vfn_pack16_size buffer), one word per pack entry
 *    (hidden layers in plan order, then the 3-channel head): the bit pattern of max |folded weight| of that entry.
 * The facade reads both and repeats a flagged call on the exact-fp32 kernels (vf_nerf_amd/nerf.py, f16x3_guard). */
int vfn_f16x3_set_status(uint32_t* status_word);
/* Clock probe of the dominant kernel.  The fused VF + rendering launch is power-limited: the shader clock it runs at is a result
 * of the launch, not a constant of the chip (1.9-2.1 GHz measured against a nominal 2.4).  After vfn_f16x3_set_clock_probe(stamps,
 * slots) every gradient-free fused launch of the calling thread (vfn_vf_render_fused16_fwd / _products / _scatter, and through them
 * vfn_render_fwd) has workgroup b < slots store two uint64 at stamps[2b], stamps[2b+1] (device memory): the shader-clock cycles
 * (s_memtime) and the 100 MHz constant-clock ticks (s_memrealtime) between its first and its last instruction.  cycles / ticks x
 * 0.1 = GHz while that workgroup ran.  NULL / 0 switches it off (the default).  Thread-local.  No reference counterpart. */
int vfn_f16x3_set_clock_probe(uint64_t* stamps, int64_t slots);
/* vfn_weight_grad_partials(shape 0, ld 256, all 256 columns valid) on the bf16 matrix cores: operands split into two
 * bf16 halves (16 significant bits, fp32 exponent range), three products per K-block, fp32 accumulation; same outputs
 * (`groups` slabs [groups][256][256] and [groups][256]).  ~2^-16 relative error per product under the sum over points. */
int vfn_weight_grad_partials_bf16(const float* dy, const float* x, int64_t n_points, int32_t groups, float* dw_part,
                                  float* db_part, int32_t x_f16, void* stream);
/* The same over 256 columns of wider matrices: rows ld_dy / ld_x floats apart (>= 256, multiples of 4, 16-byte aligned bases) — a
 * 256-column block of the rendering net's 289-wide input or of the vector-field net's 259-wide output gradient (batchstat.py). */
int vfn_weight_grad_partials_bf16_ld(const float* dy, int32_t ld_dy, const float* x, int32_t ld_x, int64_t n_points, int32_t groups,
                                     float* dw_part, float* db_part, int32_t x_f16, void* stream);
/* The same with the ACTIVATION folded into the X operand's read (round 6, ABI 5): z_prev[M, ldz] is the previous layer's pre-BatchNorm
 * output and the operand is post_prev * max(z * scale + shift, 0) on the first n_prev of the 256 columns (coef_prev = [4][n_prev]: scale |
 * shift | mean | rstd, as vfn_bstat_finalize writes them) and post_prev * z on the others (the skip layer's re-injected encoding,
 * vector_field_network.py:192-193) — vfn_bstat_relu_rows' expression value for value, so the activated matrix of a training-mode
 * layer (vector_field_network.py:146-173 under model.train()) need not exist in HBM. */
int vfn_weight_grad_partials_bf16_fold(const float* dy, int32_t ld_dy, const float* z_prev, int32_t ldz, const float* coef_prev,
                                       int32_t n_prev, float post_prev, int64_t n_points, int32_t groups, float* dw_part,
                                       float* db_part, void* stream);

/* vfn_mlp_bwd_chain on the bf16 matrix cores (split operands, three products per K-block, fp32 accumulation; shipped layer
 * shapes only, others return VFN_ERR_UNSUPPORTED).  Takes its own TRANSPOSED bf16 packs (vfn_pack_weights_bwd16; re-run
 * after every optimizer step) and the raw rows 0..2 of each net's last Linear ([3][256] fp32) for the 3-channel heads.
 * Same outputs as vfn_mlp_bwd_chain.  n_points < 2^22 per launch.
 * `masks` = the sign bits the f16x3 training forwards write next to `saved` (save_masks[13][M][2][4] u32: per slot, point and
 * lane half g one 16-byte word; tile t of the layer -> half t & 1 of dword t >> 1, bit r <-> output column
 * 32 t + (r & 3) + 8 (r >> 2) + 4 g): a ReLU's backward needs only whether its output was positive, so the chain reads
 * 32 bytes per point and layer instead of 1 KiB; `saved` itself is read only for the tanh'ed feature block (slot 8). */
int64_t vfn_packed_bwd16_size(int32_t net_kind, const vfn_net_geom* geom);                      /* bytes */
int vfn_pack_weights_bwd16(int32_t net_kind, const vfn_net_geom* geom, const vfn_layer_params* layers, void* packed,
                           void* stream);
/* The same pack with round_hi != 0: the hi planes hold the bf16 ROUNDING of the folded weights (to nearest even) instead of
 * their truncation — the pack of the single-product chain (dy_flags bit 4 below), which reads nothing else. */
int vfn_pack_weights_bwd16_mode(int32_t net_kind, const vfn_net_geom* geom, const vfn_layer_params* layers, int32_t round_hi,
                                void* packed, void* stream);
int vfn_mlp_bwd_chain_bf16(const vfn_net_geom* vf_geom, const void* vf_packed_bwd16, const float* vf_head_w,
                           const vfn_net_geom* rn_geom, const void* rn_packed_bwd16, const float* rn_head_w,
                           const float* saved, const uint32_t* masks, float* dy, const float* d_colors, const float* colors,
                           const float* d_vec, const float* vec, const float* d_feats, int32_t vec_stride,
                           int64_t n_points, float* dz_rgb, float* dz_vec, void* stream);

/* The same chain for the FRAGMENT-ORDERED workspace (below): `feats` = the tanh'ed features [M][256] row-major fp32 (the one
 * slot the chain reads as values), `dy` = the gradient slots it writes, dy_flags bit 1: fragment order, bit 2 (with bit 1):
 * as bf16, bit 3 (with bit 1, not with bit 2): as SCALED f16 (vfn_weight_grad_frag, dy_form 3).  dy_flags = 0 and feats =
 * slot 8 of saved[13][M][256] is vfn_mlp_bwd_chain_bf16.  n_points < 2^21 per LAUNCH (32-bit offsets relative to the launch's first point);
 * a workspace filled and walked by several launches (the _at forms) may hold up to 2^26 points.
 * dy_flags bit 4 (with bits 1 and 3; fused or vector-only chains): SINGLE-PRODUCT arithmetic — one bf16 product per K-block on
 * round-to-nearest operands (8 significant bits each) instead of three on split ones (16): the chain of the opt-in 16-bit-native
 * training mode (BASELINE.json configs[2], "bf16 MFMA MLPs" as written; vf_nerf_amd: model.training_products = 1).  Takes packs
 * made by vfn_pack_weights_bwd16_mode(round_hi = 1).  Outside the 1e-3 gradient bound of the default chain by construction. */
int vfn_mlp_bwd_chain_bf16_ws(const vfn_net_geom* vf_geom, const void* vf_packed_bwd16, const float* vf_head_w,
                              const vfn_net_geom* rn_geom, const void* rn_packed_bwd16, const float* rn_head_w,
                              const float* feats, const uint32_t* masks, void* dy, int32_t dy_flags, const float* d_colors,
                              const float* colors, const float* d_vec, const float* vec, const float* d_feats,
                              int32_t vec_stride, int64_t n_points, float* dz_rgb, float* dz_vec, void* stream);
/* The same over PART of a workspace sized for ws_points points: the launch's n_points points are points ws_first .. of feats,
 * masks, dy, dz_rgb and dz_vec (workspace-indexed); d_colors / colors / d_vec / vec / d_feats stay launch-local.  Several
 * forwards can then share one workspace (vfn_vf_render_fused16_fwd_train_at, vfn_vf_mlp16_fwd_train_at) and the weight-gradient
 * kernels walk it once. */
int vfn_mlp_bwd_chain_bf16_ws_at(const vfn_net_geom* vf_geom, const void* vf_packed_bwd16, const float* vf_head_w,
                                 const vfn_net_geom* rn_geom, const void* rn_packed_bwd16, const float* rn_head_w,
                                 const float* feats, const uint32_t* masks, void* dy, int32_t dy_flags, const float* d_colors,
                                 const float* colors, const float* d_vec, const float* vec, const float* d_feats,
                                 int32_t vec_stride, int64_t n_points, float* dz_rgb, float* dz_vec, int64_t ws_first,
                                 int64_t ws_points, void* stream);

/* FRAGMENT-ORDERED training workspace.  A slot (one layer's saved activations, or its pre-activation gradients) is stored as
 * the producing waves hold it: groups of 32 points (one wave), 32 KiB per group, inside a group piece (t, q) = registers
 * 4q..4q+3 of output tile t at byte (4 t + q) * 1024 (512 in 16-bit forms), inside a piece lane L = 32 g + i at L * 16 (8)
 * bytes holding columns 32 t + 8 q + 4 g .. + 3 of point 32 G + i.  Every store of the f16x3 training forward / the bf16
 * chain and every load of the weight-gradient kernel is then 1 KiB (512 B) of consecutive bytes; row-major slots made each
 * store touch 32 lines with 32 (16) bytes.  Slot stride = ceil(M / 32) * 32 KiB whatever the element size.
 * vfn_weight_grad_frag: the weight-gradient partial slabs of vfn_weight_grad_partials (same `groups` slabs, same shapes
 * 0: [256][256], 1: [256][64], 2: [32][256], db_part [groups][256 | 256 | 32]) from such slots, split-bf16 products on
 * v_mfma_f32_32x32x16_bf16:
 *   dy_form 0 fragment fp32 | 1 fragment bf16 (no low half: two products per K-block) | 2 dz[M][4] fp32 rows (shape 2 only)
 *           3 fragment SCALED f16: the 16 values lane L holds of tile t are f16(dY * 2^k), k chosen by the producer so that the
 *             largest magnitude lies in [2^14, 2^15) (11 significant bits at any gradient scale); pieces where the bf16 form has
 *             them, the byte k + 113 (255: all zero) at byte 16384 + 64 t + L of the group.  The kernel brings a slab's pieces to
 *             one common scale and multiplies on v_mfma_f32_32x32x16_f16: one product per K-block with f16 activations (x_form 1),
 *             two with fp32 ones (f16 hi + lo)
 *   x_form  0 fragment fp32 | 1 fragment f16 | 2 [M][256] fp32 rows (the features) | 3 the encoding tile aux[M][40] (shape 1 only)
 * Points past M in the last group count as zero. */
int vfn_weight_grad_frag(int32_t shape, const void* dy, int32_t dy_form, const void* x, int32_t x_form, int64_t n_points,
                         int32_t groups, float* dw_part, float* db_part, void* stream);

/* Split inference launches.  The reference evaluates the vector-field net on every proposal sample twice (no-grad pass
 * vector_field_nerf.py:252-277, then again among the S_c+N_f samples at :294-297); the two entry points below let a caller
 * evaluate it once per distinct sample and run the rendering net on gathered results — same arithmetic per sample as
 * vfn_vf_render_fused16_fwd, so the outputs are identical.
 * vfn_vf_feat16_fwd: points[M,3] -> out_vec[M,3] (tanh'ed vector columns) and out_blocks, the 256 tanh'ed features in the
 *   rendering kernel's operand format (split f16): 32 KiB per group of 32 consecutive rows,
 *   [operand block 0..15][hi | lo][lane 0..63][16 B], i.e. the register image of the wave that owns those rows — every store
 *   and every later load moves 1 KiB of consecutive bytes.  The buffer holds ceil(M / 32) groups (rows past M in the last
 *   group are written with don't-care values); a launch must start on a group boundary of the buffer.  M < 2^22.
 * vfn_render16_from_blocks: the rendering net over the n_rows stored rows, in storage order: row r has its features in
 *   blocks, its vector columns in vecs[r], and dst[r] = its position among the sorted samples of the batch
 *   (vfn_range_fine_sample_indexed produces dst; dst[r] < 0 marks a padding row): position points[dst[r]], view direction
 *   ray_dirs[dst[r] / S]; writes normals[dst[r]] (= vecs[r]) and colors[dst[r]].  The rendering net is pointwise, so the
 *   result equals vfn_vf_render_fused16_fwd on the sorted samples. */
int vfn_vf_feat16_fwd(const vfn_net_geom* geom, const void* packed16, const float* points, int64_t n_points,
                      float* out_vec, void* out_blocks, void* stream);
/* out_a[index[r]] = a[r] (and out_b[index[r]] = b[r] when b != NULL) for [n_rows,3] fp32 rows; negative indices are skipped.
 * Moves per-sample results computed in generation order to their positions among the sorted samples. */
int vfn_scatter_rows3(const float* a, const float* b, const int32_t* index, int64_t n_rows, float* out_a, float* out_b,
                      void* stream);
/* vfn_vf_render_fused16_fwd whose outputs of point m go to row out_index[m] of normals / colors (negative: dropped): the
 * N_f new samples of the split pipeline need no block round trip at all — they run the fused launch in generation order
 * (view direction of point m = ray_dirs[m / samples_per_ray]) and land at their sorted positions. */
int vfn_vf_render_fused16_scatter(const vfn_net_geom* vf_geom, const void* vf_packed16, const vfn_net_geom* rn_geom,
                                  const void* rn_packed16, const float* points, const float* ray_dirs, int64_t n_points,
                                  int32_t samples_per_ray, const int32_t* out_index, float* normals, float* colors,
                                  void* stream);
/* The fused launch with the number of f16 products per fp32-equivalent product of its COLOUR BRANCH (the feature block of the
 * vector-field net and the whole rendering net) chosen by the caller: colour_products = 3 is vfn_vf_render_fused16_fwd /
 * _scatter; 2 evaluates that branch as w_hi x_hi + w_hi x_lo — weights as their f16 roundings, activations still split — which
 * removes 14 % of the launch's matrix instructions and a third of its weight traffic.  The vector head and every layer before
 * it keep three products, so normals (hence density, weights, depth, sample positions) are bit-identical to the 3-product
 * launch; colours differ from the reference by <= 2e-5 on its golden outputs (contract: 1e-4).  out_index: NULL (outputs in
 * place) or the scatter index.  Same packs as every other f16x3 entry point. */
int vfn_vf_render_fused16_products(const vfn_net_geom* vf_geom, const void* vf_packed16, const vfn_net_geom* rn_geom,
                                   const void* rn_packed16, const float* points, const float* ray_dirs, int64_t n_points,
                                   int32_t samples_per_ray, const int32_t* out_index, int32_t colour_products, float* normals,
                                   float* colors, void* stream);
int vfn_render16_from_blocks(const vfn_net_geom* rn_geom, const void* rn_packed16, const void* blocks, const float* vecs,
                             const int32_t* dst, const float* points, const float* ray_dirs, int64_t n_rows,
                             int32_t samples_per_ray, float* normals, float* colors, void* stream);

/* From partial slabs to parameter gradients, all layer entries of a net in one launch: sums the `groups` slabs written
 * by vfn_weight_grad_partials(_bf16) and un-folds eval-mode BatchNorm and the skip scale (W' = s scale W,
 * b' = s (b - mu) + beta, s = gamma / sqrt(var + 1e-5)) onto the parameters the optimizer holds:
 * rows [row_off, row_off + rows) of g_w[out][in_dim] (columns act_c0.. and aux_c0..), g_b, and, with BatchNorm, g_bn_w, g_bn_b.
 * slab_rows = rows per slab group (256, or 32 for the 3-channel head).  At most 12 entries. */
typedef struct {
    const float* dw_act; const float* dw_aux; const float* db;
    const float* w; const float* b_lin; const float* bn_w; const float* bn_var; const float* bn_mean;
    float* g_w; float* g_b; float* g_bn_w; float* g_bn_b;
    int32_t rows, row_off, in_dim, slab_rows;
    int32_t act_c0, act_nc, aux_c0, aux_nc;
    float scale;
    int32_t groups_act, groups_aux, groups_db;   /* slabs of dw_act / dw_aux / db of THIS entry; 0: the call's `groups` (products batched
                                                  * into one launch, csrc/vfn_wgrad.hip, have fewer slabs than single ones) */
} vfn_unfold_entry;
int vfn_unfold_weight_grads(const vfn_unfold_entry* entries, int32_t n_entries, int32_t groups, void* stream);
/* The same with bit i of accumulate_mask saying that entry i ADDS its result to what g_w / g_b / g_bn_w / g_bn_b already hold:
 * the targets are then the parameters' own .grad tensors, and autograd's ~90 per-parameter accumulation kernels per training
 * step are not launched at all. */
int vfn_unfold_weight_grads_acc(const vfn_unfold_entry* entries, int32_t n_entries, int32_t groups, uint32_t accumulate_mask,
                                void* stream);

/* The parameter gradients of ONE network from a fragment-ordered workspace in ONE call (csrc/vfn_wgrad.hip): the
 * vfn_weight_grad_frag launches of every layer entry (activation columns, encoding columns), of the 3-channel head, and the
 * vfn_unfold_weight_grads_acc launch, issued on `stream` out of `scratch` (vfn_net_weight_grads_scratch_bytes; no allocation, no
 * synchronisation) — loss.backward() through vector_field_network.py:177-208 / rendering_network.py:62-108
 * (train/vector_field_nerf_train.py:252) after the dX chain has written the gradient slots.
 *   layers[geom->n_layers]: the reference's parameters per nn.Linear (+ BatchNorm1d) and where their gradients go;
 *   saved / dy: THIS net's first activation / gradient slot (slot stride slot_bytes = ceil(M/32) * 32 KiB);
 *   dy_form / x_form as in vfn_weight_grad_frag; feats: the tanh'ed features [M][256] fp32 rows (rendering net: input of its
 *   first layer; vector-field net: unused, may be NULL); aux: this net's encoding tile [M][40]; dz_head: [M][4];
 *   with_features = 0 (vector-field net only): the forward was vector-only, the feature block's rows get no gradient;
 *   accumulate != 0: results are ADDED to the gradient tensors (they are the parameters' .grad), else written.
 * vfn_weight_grad_groups(M) = the number of partial slabs per product the entry points use for M points. */
typedef struct vfn_wgrad_layer {
    const float* weight; const float* bias; const float* bn_weight; const float* bn_var; const float* bn_mean;
    float* g_weight; float* g_bias; float* g_bn_weight; float* g_bn_bias;
} vfn_wgrad_layer;
/* ... and the same for a SUBSET of the net's products: parts = VFN_WGRAD_LAYERS (the hidden layers) | VFN_WGRAD_FEATURES (the
 * feature block of the vector-field net's last Linear) | VFN_WGRAD_HEAD (its 3 output channels).  One workspace can hold points
 * whose forward included the feature block (the fine pass of render()) followed by points whose forward did not (the trainer's
 * supervision points, vector_field_nerf_train.py:191,203,215): LAYERS | HEAD then run once over all of them, FEATURES over the
 * first block only (pointers of a sub-range of points: slot base + (first / 32) * 32 KiB, aux + first * 40, dz_head + first * 4). */
#define VFN_WGRAD_LAYERS 1u
#define VFN_WGRAD_FEATURES 2u
#define VFN_WGRAD_HEAD 4u
int vfn_net_weight_grads_frag_part(int32_t net_kind, const vfn_net_geom* geom, const vfn_wgrad_layer* layers, const void* saved,
                                   const void* dy, int64_t slot_bytes, int32_t dy_form, int32_t x_form, const float* feats,
                                   const float* aux, const float* dz_head, int64_t n_points, uint32_t parts, int32_t accumulate,
                                   void* scratch, void* stream);
int32_t vfn_weight_grad_groups(int64_t n_points);
int64_t vfn_net_weight_grads_scratch_bytes(int32_t net_kind, const vfn_net_geom* geom, int64_t n_points);
int vfn_net_weight_grads_frag(int32_t net_kind, const vfn_net_geom* geom, const vfn_wgrad_layer* layers, const void* saved,
                              const void* dy, int64_t slot_bytes, int32_t dy_form, int32_t x_form, const float* feats,
                              const float* aux, const float* dz_head, int64_t n_points, int32_t with_features,
                              int32_t accumulate, void* scratch, void* stream);

/* VFLoss (models/losses/vf_loss.py:34-87) and the trainer's centre-ball selection (models/helpers/functions.py:137-157,
 * train/vector_field_nerf_train.py:203-214) fused (csrc/vfn_loss.hip): vfn_vf_loss_fwd = one reduction launch + a one-workgroup finish
 * -> out_terms[8] = {rgb, depth, unit_norm, supervision, norm_smaller_than_one, 0 (the directional-derivative term stays with the
 * caller), weighted total of the five, supervision rows}; vfn_vf_loss_bwd = one elementwise launch writing d total / d inputs times
 * the device scalar grad_out (NULL: 1).  rgb[N,3], depth[N] (has_depth), normals[M,3]; up to three supervision segments
 * sup_pred[k][n_sup[k],3] / sup_gt[k] (host arrays of three device pointers); ray_center != 0: the rows of `normals` whose point
 * (`points`[M,3]) lies within `radius` of `centroid` form a fourth segment with ground truth normalize(point - centroid) — selected
 * and counted on the device, no compaction, no host synchronisation.  `workspace`: vfn_vf_loss_workspace_bytes() bytes, written by
 * the forward call and read by the backward call (the supervision mean's data-dependent denominator lives there). */
typedef struct vfn_loss_params {
    int64_t n_rays, n_normals;
    int64_t n_sup[3];
    int32_t has_depth;       /* 0: no depth term (the batch has no depth ground truth) */
    int32_t smaller_on;      /* epoch >= norm_smaller_than_one_start */
    int32_t ray_center;
    int32_t reserved;
    float w_rgb, w_depth, w_unit, w_sup, w_smaller;
    float depth_clamp;
    float radius;
    float centroid[3];
} vfn_loss_params;
int64_t vfn_vf_loss_workspace_bytes(void);
int vfn_vf_loss_fwd(const vfn_loss_params* p, const float* rgb, const float* rgb_gt, const float* depth, const float* depth_gt,
                    const float* normals, const float* points, const float* const* sup_pred, const float* const* sup_gt,
                    void* workspace, float* out_terms, void* stream);
int vfn_vf_loss_bwd(const vfn_loss_params* p, const float* rgb, const float* rgb_gt, const float* depth, const float* depth_gt,
                    const float* normals, const float* points, const float* const* sup_pred, const float* const* sup_gt,
                    const void* workspace, const float* grad_out, float* d_rgb, float* d_depth, float* d_normals,
                    float* const* d_sup, void* stream);

/* Supervision points of the trainer (train/vector_field_nerf_train.py:186-214): n uniform samples in the spherical
 * shell r_min <= |p - centroid| <= r_max (models/samplers/sampler.py:160-193) and their radial unit ground truth
 * (models/helpers/functions.py:100-135): inward = 1 -> normalize(centroid - p) (sample_border_points), 0 -> normalize(p -
 * centroid) (sample_center_points).  u[n,3] supplies the three uniforms per sample (parity runs) or is NULL (Philox). */
int vfn_sample_sphere_shell(int64_t n, float r_min, float r_max, const float* centroid, int32_t inward, const float* u,
                            uint64_t seed, uint64_t offset, float* points, float* gt, void* stream);

/* The same forwards under autograd (train/vector_field_nerf_train.py:177,191,203,215): they additionally fill the
 * workspace the backward entry points read (`saved` slots, save_aux_vf[M,40], save_aux_rn[M,40]; see "slots" above),
 * exactly like vfn_vf_mlp_fwd_train / vfn_vf_render_fused_fwd_train.  with_features = 0 evaluates only the vector head
 * (the feature slot is not written); with_features = 1 also writes the 256 tanh'ed features into their slot, from which
 * the caller assembles [M, 3+F].  n_points < 2^22 per launch.
 * save_masks: the sign bits of every saved ReLU output (see vfn_mlp_bwd_chain_bf16).  save_f16 = flags.  Bit 0: the ReLU slots
 * are stored as f16 — 256 values in the first 512 bytes of every 1 KiB row, the row stride does not change — which halves
 * what the forward writes and the weight-gradient kernels read, at 11 instead of 24 significant bits in the activations that
 * multiply dY (BASELINE.json configs[2] trains on bf16 matrix cores); the tanh'ed feature slot (8) stays fp32 row-major.
 * Bit 1: the ReLU slots are FRAGMENT-ORDERED (see vfn_weight_grad_frag; slot stride ceil(M/32) * 32 KiB, n_points < 2^21 per launch, ws_points < 2^26).
 * Bit 2 (vfn_vf_mlp16_fwd_train[_at] with with_features = 0; the fused launch takes colour_products = 1 instead): SINGLE-PRODUCT
 * arithmetic — every K-block is ONE f16 product of the operands' f16 roundings (11 significant bits each, fp32 accumulation)
 * instead of three on split operands: the forward of the opt-in 16-bit-native training mode (BASELINE.json configs[2], "bf16
 * MFMA MLPs" as written — f16 keeps three more bits at the same matrix rate).  Same pack (its hi planes), same workspace; the
 * outputs are ~1e-3 from the fp32 ones, i.e. OUTSIDE the 1e-4 contract: never a default, never used by gradient-free renders. */
int vfn_vf_mlp16_fwd_train(const vfn_net_geom* geom, const void* packed16, const float* points, int64_t n_points,
                           int32_t with_features, float* out_vec, float* saved, float* save_aux_vf, uint32_t* save_masks,
                           int32_t save_f16, void* stream);
int vfn_vf_mlp16_fwd_train_at(const vfn_net_geom* geom, const void* packed16, const float* points, int64_t n_points,
                              int32_t with_features, float* out_vec, float* saved, float* save_aux_vf, uint32_t* save_masks,
                              int32_t save_f16, int64_t ws_first, int64_t ws_points, void* stream);    /* see ..._fused16_fwd_train_at */
int vfn_vf_render_fused16_fwd_train(const vfn_net_geom* vf_geom, const void* vf_packed16, const vfn_net_geom* rn_geom,
                                    const void* rn_packed16, const float* points, const float* ray_dirs,
                                    int64_t n_points, int32_t samples_per_ray, float* normals, float* colors,
                                    float* saved, float* save_aux_vf, float* save_aux_rn, uint32_t* save_masks, int32_t save_f16,
                                    void* stream);
/* The same launch filling PART of a workspace sized for ws_points points: its n_points points are points ws_first ..
 * ws_first + n_points - 1 of every slot, of the sign-bit words and of the encoding tiles (outputs normals / colors stay
 * launch-local, [n_points,3]).  A training render evaluates the vector-field net once per distinct sample this way: the proposal
 * samples (vector_field_nerf.py:252-256) and, after the fine sampler, the new samples (:294-297) fill ONE workspace in storage
 * order, which the chain and the weight-gradient kernels then walk once.  ws_first % 32 == 0 in fragment order.
 * colour_products: 3, or 2 = the colour branch of THIS forward on two products (vfn_vf_render_fused16_products): the loss sees
 * colours 2e-5 off, the saved activations move by less than their f16 storage rounds them, the backward is unchanged;
 * 1 = ONE product everywhere (see save_f16 bit 2 above). */
int vfn_vf_render_fused16_fwd_train_at(const vfn_net_geom* vf_geom, const void* vf_packed16, const vfn_net_geom* rn_geom,
                                       const void* rn_packed16, const float* points, const float* ray_dirs,
                                       int64_t n_points, int32_t samples_per_ray, float* normals, float* colors,
                                       float* saved, float* save_aux_vf, float* save_aux_rn, uint32_t* save_masks,
                                       int32_t save_f16, int64_t ws_first, int64_t ws_points, int32_t colour_products, void* stream);

/* =============================================================================================
 * Dense-grid stages between the vector-field queries and the mesh triangulation (evaluation/utils/mc_utils.py,
 * evaluation/utils/guassian_smoothing.py).  Grid cell (i,j,k) -> (i n + j) n + k; field vt[n^3,3]; n <= 1024.
 * ============================================================================================= */
/* evaluation/methods.py:194-208 fills samples[n^3,3] on the host with a SEPARABLE lattice: column 0 of cell (i,j,k) depends on i alone,
 * column 1 on j, column 2 on k (index * voxel_size + origin + translation + centroid, in fp32).  Given the three axis tables
 * axis0[n], axis1[n], axis2[n] (device; the caller reads them off the host tensor's first row / column / plane), writes
 * points[count,3] = rows [row0, row0 + count) of that grid — the caller's values bit for bit — so the 12 B per point of
 * mc_utils.get_set_predictions' upload (mc_utils.py:96-97) never crosses PCIe.  n <= 2048. */
int vfn_grid_lattice_points(const float* axis0, const float* axis1, const float* axis2, int32_t n, int64_t row0, int64_t count,
                            float* points, void* stream);
/* mc_utils.py:34-86: out[n^3] = 1 where the flux of the normalised field through the cell's 8 corners is <= threshold
 * (-0.5 in the reference), else 0; cells of the last planes are 0. */
int vfn_grid_divergence(const float* vt, int32_t n, float threshold, float* out, void* stream);
/* guassian_smoothing.py:81-97: one axis of the separable Gaussian (k odd, <= 15 host weights), replicate padding;
 * three calls (axis 0, 1, 2) = smooth_vf.  Out of place. */
int vfn_grid_smooth_axis(const float* in, float* out, int32_t n, int32_t axis, const float* weights_host, int32_t k,
                         void* stream);
/* mc_utils.py:107-167: for cells with divergence == 1, which of the cell's two most opposed corner vectors each of the 8
 * corners sides with (0/1; corner order (0,0,0) (0,1,0) (1,1,0) (1,0,0) (0,0,1) (0,1,1) (1,1,1) (1,0,1)); other cells 0.
 * vt is the normalised field [n^3,3]. */
int vfn_grid_unify_direction(const float* divergence, const float* vt, int32_t n, int64_t* choice, void* stream);
/* mc_utils.py:170-223: for the 28 corner pairs (a<b) of every cell: different_side[n^3,28] = choice_a != choice_b,
 * pair_norms[n^3,28,2] = (norms at corner a, norms at corner b), corners outside the grid read as 0. */
int vfn_grid_comb_format(const int64_t* choice, const float* norms, int32_t n, float* different_side, float* pair_norms,
                         void* stream);
/* The same two stages with the side bits of a cell as ONE byte (bit q = corner q's side): `sides`[n^3] is written beside (choice
 * != NULL) or instead of (choice == NULL) the int64 table, and vfn_grid_comb_format_sides reads it instead of 64 B per cell.  What
 * evaluation/methods.py:248-253 does with the table — hand it to make_comb_format and delete it — needs nothing else. */
int vfn_grid_unify_direction_sides(const float* divergence, const float* vt, int32_t n, uint8_t* sides, int64_t* choice, void* stream);
int vfn_grid_comb_format_sides(const uint8_t* sides, const float* norms, int32_t n, float* different_side, float* pair_norms,
                               void* stream);

/* =============================================================================================
 * Mesh triangulation: contrastive marching cubes (evaluation/utils/marching_cubes_vt.py:186-315 with combs_to_verts :62-101 and
 * vertex_interpolate :9-16), the stage after make_comb_format in evaluation/methods.py:256-291.  Four stream-ordered calls:
 *   vfn_mesh_count   per cell POSITION p < m: triangle count counts[p]; offsets[p] = inclusive scan of counts; info[0] = triangles T,
 *                    info[1] |= 1 (a non-finite corner value / norm, see below) | 2 (a cell index outside [0, res)).  The caller
 *                    zero-fills info[4] first and reads it back once to size the outputs.
 *   vfn_mesh_emit    tri_verts[3 T, 3] (double): the corners of every triangle at slot 3 (offsets[p] - counts[p] + t) + corner.
 *   vfn_mesh_dedup   vertices with equal (x, y, z) — compared as doubles: 0.0 == -0.0 — share one id, owned by the smallest slot;
 *                    table / owner: table_size (a power of two >= 2 x n_slots) int32 each, bucket / flags / vid: n_slots int32 each;
 *                    info[2] = unique vertices V.  Result independent of the order in which the device's atomics arrive.
 *   vfn_mesh_number  vertices[V, 3] (double, the first occurrence's bits) in order of first appearance and faces[n_slots] (int64,
 *                    0-based ids: the reference's fs - 1).
 * Cell positions, the reference's visiting order:
 *   VFN_MESH_GENERAL comb[m, 28] (+ udf[m, 28, 2] or NULL: corner values 0 / 1), fp32 (f64 = 0) or fp64 (f64 = 1), position p = the
 *                    cell cells[p] (int64 [m, 3]) or, cells == NULL, the dense raster (m = res^3, p = (i res + j) res + k).  Any comb
 *                    table: anchors by first argmax, strict comparisons, as combs_to_verts.  A NaN in a comb row: no triangles (np.max
 *                    is NaN).  Corner values from udf that are not finite in a cell with cut edges set info[1] bit 1.
 *   VFN_MESH_FUSED   sides[res^3] (the side byte per cell of vfn_grid_unify_direction_sides) + norms[res^3] (fp32): the positions
 *                    are the (res/2)^3 blocks of 2x2x2 cells of methods.py:184-188 in raster order, cells inside a block in corner
 *                    order; value of corner v = (bit_v != bit_0 ? +1 : -1) x norm(corner v), norm 0 outside the grid — what
 *                    make_comb_format's XOR table and pair norms give combs_to_verts.  res even, <= 1024; any non-finite norm in the
 *                    grid sets info[1] bit 1.
 * Corner positions (i / res) x size - size / 2 in fp64; all arithmetic fp64 without contraction.  Limits: m < 2^31, 3 T < 2^31.
 * ============================================================================================= */
#define VFN_MESH_GENERAL 0
#define VFN_MESH_FUSED 1
/* Host copies of the embedded tables: edge_table[256] (cut-edge masks), edge_vertex[12 x 2] (marching_cubes_lookup.EDGE_VERTEX order),
 * tri_table[256 x 16] (int8, -1 padded). */
int vfn_mesh_tables(int32_t* edge_table, int32_t* edge_vertex, int8_t* tri_table);
/* Device workspace (bytes) of the scan over n int32 values that vfn_mesh_count / vfn_mesh_dedup run; -1 on error. */
int64_t vfn_mesh_scan_workspace_bytes(int64_t n);
int vfn_mesh_count(int32_t form, const void* comb, const void* udf, int32_t f64, const int64_t* cells, const uint8_t* sides,
                   const float* norms, int64_t m, int32_t res, double size, double isovalue, int32_t* counts, int32_t* offsets,
                   int64_t* info, void* scan_ws, int64_t scan_ws_bytes, void* stream);
int vfn_mesh_emit(int32_t form, const void* comb, const void* udf, int32_t f64, const int64_t* cells, const uint8_t* sides,
                  const float* norms, int64_t m, int32_t res, double size, double isovalue, const int32_t* counts,
                  const int32_t* offsets, double* tri_verts, void* stream);
int vfn_mesh_dedup(const double* tri_verts, int64_t n_slots, int32_t* table, int32_t* owner, int64_t table_size, int32_t* bucket,
                   int32_t* flags, int32_t* vid, int64_t* info, void* scan_ws, int64_t scan_ws_bytes, void* stream);
int vfn_mesh_number(const double* tri_verts, int64_t n_slots, const int32_t* owner, const int32_t* bucket, const int32_t* vid,
                    double* vertices, int64_t* faces, void* stream);
/* evaluation/methods.py:223-226 for field[n, 3]: norms[n] = torch.norm(field, dim=1) bit for bit with torch's CPU kernel
 * (sqrt(fma(z, z, fma(y, y, x x))), correctly rounded) and, unit != NULL, unit[n, 3] = F.normalize(field, dim=1) = field / max(norm, 1e-12). */
int vfn_mesh_field_norms(const float* field, int64_t n, float* norms, float* unit, void* stream);

/* =============================================================================================
 * Scoring a mesh against a mesh (csrc/vfn_metrics.hip): the geometry of evaluation/methods.py:747-801 (metrics_3d_no_vf) with
 * utils/utils.py:327-367 (get_chamfer_distance) — area-weighted surface samples, every sample's nearest neighbour in the other set,
 * statistics of the distances.  Everything is float64, evaluated without contraction in the association written here, and no result
 * depends on the order in which workgroups or atomics arrive.  `info` words are zero-filled by the caller and only ever OR-ed into:
 * bit 1 = a non-finite value, bit 2 = a face index outside [0, V).  Limits: every count < 2^31.
 *   vfn_nn_sqdist     reads queries[n, 3], targets[m, 3] (row-major); writes best[n] = min over j of ((dx dx + dy dy) + dz dz) with
 *                     dx = q.x - t_j.x, dy = q.y - t_j.y, dz = q.z - t_j.z — the SQUARED distance to the nearest target; the caller
 *                     takes sqrt (monotone and correctly rounded: sqrt of the minimum is the minimum of the sqrts).  All n x m pairs
 *                     are evaluated (no spatial structure, no index output).  best is filled with +inf by the same call; the target
 *                     slices of one query merge with an integer atomicMin on the bits of the non-negative double.  info[0] |= 1 when
 *                     a coordinate of either set is not finite (best is then meaningless).  1 <= n, m < 2^31.
 *   vfn_tri_areas     reads vertices[V, 3], faces[F, 3] (int64); writes areas[F] = 0.5 sqrt((c.x c.x + c.y c.y) + c.z c.z) with
 *                     e1 = v1 - v0, e2 = v2 - v0, c = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x), both
 *                     products of a component rounded.  A face with an index outside [0, V): info[0] |= 2, area 0.  A non-finite
 *                     area: info[0] |= 1.
 *   vfn_cumsum_f64    out[i] = x[0] + ... + x[i] as a FIXED tree: blocks of 1024 values (a lane adds 4 values serially, a
 *                     Kogge-Stone scan over the 256 lane totals, one addition of the lane's own prefix), the block totals scanned
 *                     the same way, one addition per level on the way down — a prefix is at most 12 x levels additions deep,
 *                     levels = 1 for n <= 1024, 2 for n <= 1024^2, 3 for n <= 1024^3, 4 above.  The bits are a function of n and the data alone (a
 *                     look-back scan's are not), so equal uniforms always select equal faces.  Neighbouring prefixes are rounded
 *                     along different paths: the output may step down by an ulp (the caller that needs a monotone table takes a
 *                     running maximum, which is exact).  x and out may be the same array.
 *                     workspace: vfn_cumsum_workspace_bytes(n) bytes of device memory (0 for n <= 1024); -1 on error.
 *   vfn_sample_surface  reads vertices, faces, cum[F] (the inclusive cumulative areas, non-decreasing) and uniforms[count, 3] in [0, 1);
 *                     point i: t = u[i,0] cum[F-1]; face = the smallest index with cum[face] > t (binary search), clamped to F - 1 — a
 *                     zero-area face is never chosen; a = u[i,1], b = u[i,2], and if a + b > 1 then a = 1 - a, b = 1 - b;
 *                     points[i, c] = (v0[c] + a e1[c]) + b e2[c] with e1 = v1 - v0, e2 = v2 - v0.  Writes points[count, 3] and
 *                     face_index[count] (int64).  A chosen face with an index outside [0, V): info[0] |= 2, point 0.
 *   vfn_reduce_stats  reads x[n]; writes stats[4] = sum, min, max, number of x[i] < threshold (as a double: exact), each along THE FIXED
 *                     TREE below with the lane order "far"; values past n join as the identity.
 *                     workspace: vfn_reduce_stats_workspace_bytes(n) bytes (the partials); -1 on error.
 *
 * THE FIXED TREE (csrc/vfn_tree.h) joins the sums of vfn_reduce_stats, vfn_icp_accumulate, vfn_image_scores and vfn_image_abs_err: two
 * launches, no floating-point atomics, the bits a function of the sizes and the data alone.  A join of two values puts the value of the
 * lower slot, lane or partial on the left.
 *   Tile.  Block b owns the VFN_TREE_LANES x VFN_TREE_PER = 256 x 16 = 4096 values [4096 b, 4096 (b + 1)); lane l owns the value
 *   4096 b + l + 256 k in its slot k, k < 16.  A value past n is the identity: +0.0 for a sum, +inf for a minimum, -inf for a maximum,
 *   0 for a count.  (The image sums have no slots: a tile is 16 x 16 pixels and a lane owns one value, see there.)
 *   Lane tree.  A lane joins its 16 slots as a balanced tree of 4 levels, in one of two orders, named by the slots that meet first:
 *     "near"  slot k with slot k + 1: ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)), ... — vfn_icp_accumulate;
 *     "far"   slot k with slot k + 8: ((v0 + v8) + (v4 + v12)) + ((v2 + v10) + (v6 + v14)), ... — the "near" tree over the slots in
 *             4-bit bit-reversed order 0, 8, 4, 12, 2, 10, 6, 14, 1, 9, ... — vfn_reduce_stats.
 *   Block tree.  The 256 lane values join as a balanced tree of 8 levels: lane l takes lane l + d for d = 128, 64, ... 1.  Lane 0's value
 *   is the block's partial; the partials lie in the workspace in block order.
 *   Second level.  One block of VFN_TREE_TOP = 1024 lanes joins the P partials: lane l starts from partial l (the identity if l >= P),
 *   joins the partials l + 1024, l + 2048, ... serially in that order, then the block tree over 1024 lanes (d = 512 ... 1, 10 levels).
 *   Depth.  A sum is (lane levels) + 8 + (ceil(P / 1024) - 1) + 10 additions deep; lane levels = 4 with P = ceil(n / 4096) for
 *   vfn_reduce_stats and vfn_icp_accumulate, C - 1 with P = the tiles of a view for the image sums.
 * ============================================================================================= */
#define VFN_TREE_LANES 256            /* lanes of a first-level block of the fixed tree */
#define VFN_TREE_PER 16               /* values a lane owns */
#define VFN_TREE_TOP 1024             /* lanes of the second level */
int vfn_nn_sqdist(const double* queries, int64_t n, const double* targets, int64_t m, double* best, int64_t* info, void* stream);
int vfn_tri_areas(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, double* areas, int64_t* info,
                  void* stream);
int64_t vfn_cumsum_workspace_bytes(int64_t n);
int vfn_cumsum_f64(const double* x, int64_t n, double* out, void* workspace, int64_t workspace_bytes, void* stream);
int vfn_sample_surface(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, const double* cum,
                       const double* uniforms, int64_t count, double* points, int64_t* face_index, int64_t* info, void* stream);
int64_t vfn_reduce_stats_workspace_bytes(int64_t n);
int vfn_reduce_stats(const double* x, int64_t n, double threshold, double* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* =============================================================================================
 * Aligning two point sets (csrc/vfn_icp.hip): the device half of point-to-point ICP, the `icp_align` step of evaluation/methods.py:747-801
 * that the reference leaves to an external package.  A SPECIFICATION, not a recording: neither Open3D nor that package publishes its
 * arithmetic.  Everything is float64, evaluated without contraction in the association written here; no result depends on the order
 * in which workgroups arrive.  `info` as above: zero-filled by the caller, bit 1 = a non-finite coordinate, bit 2 = an index outside
 * [0, m).  1 <= n, m < 2^31.
 *   A transform is 12 doubles in HOST memory, r00 r01 r02 r10 .. r22 (row-major) then t0 t1 t2; NULL is the identity and skips the
 *   arithmetic (q' = q to the bit).  Otherwise q'x = ((r00 x + r01 y) + r02 z) + t0, q'y and q'z alike with rows 1 and 2.  The points
 *   are transformed on the fly and never rewritten.  A non-finite entry is refused before any launch.
 *   vfn_transform_points  out[n, 3] = q' for points[n, 3], one lane per point.
 *   vfn_nn_radius     for every query i: among the targets j with d2(j) <= rr, where d2(j) = (dx dx + dy dy) + dz dz, dx = q'x - t_j.x,
 *                     dy = q'y - t_j.y, dz = q'z - t_j.z and rr = radius radius (rounded once), the minimum of d2, ties to the LOWEST
 *                     target index: index[i] = that j, sqdist[i] = its d2; no such target: index[i] = -1, sqdist[i] = +inf.  radius
 *                     must be finite and > 0 with a normal square.  The definition does not mention a grid and the grid does not
 *                     change a bit of the result; it only bounds the work.  The caller provides it: box[7] (HOST memory) = the
 *                     targets' componentwise minimum o[3], their maximum e[3], the cell edge h >= radius (1 + 2^-20) with
 *                     (e - o) / h <= 129 on every axis; nx, ny, nz in [1, VFN_ICP_GRID_CAP = 128] cells; with
 *                       cell(x) = min(max(floor((min(max(x, o), e) - o) / h), 0), dim - 1)    per axis,
 *                       key = (cell_x ny + cell_y) nz + cell_z,
 *                     sorted_targets[m, 3] = the targets in ascending key order, perm[m] = their original indices (what `index`
 *                     reports), cell_start[nx ny nz + 1] (int32) = the first sorted position of every key, cell_start[last] = m.
 *                     The argument that the 27 cells around a query's cell hold every admissible target under this rounding is in
 *                     csrc/vfn_icp.hip.  order[n] (may be NULL) is a permutation of the queries: lane k serves query order[k]
 *                     (neighbouring lanes then read neighbouring cells); it changes no bit.  check_finite != 0: info[0] |= 1 when a
 *                     coordinate of either set is not finite (the outputs are then meaningless); 0 skips that pass over the
 *                     3 (n + m) coordinates — for a caller that searches the same two arrays again (the ICP loop checks once).
 *   vfn_icp_accumulate  reads queries[n, 3], the transform, targets[m, 3] (ORIGINAL order), index[n], sqdist[n] and anchor[3] (HOST
 *                     memory); writes sums[17] over the rows with index[i] >= 0, with p = q'_i - anchor and s = t_index[i] - anchor
 *                     (each difference rounded once):
 *                       sums[0] = the number of rows (exact), sums[1] = sum sqdist[i], sums[2 + a] = sum p_a, sums[5 + a] = sum s_a,
 *                       sums[8 + 3 a + b] = sum p_a s_b (the product rounded once).
 *                     Every sum goes along THE FIXED TREE (above, after vfn_reduce_stats) over the n rows with the lane order "near"
 *                     — not the order of vfn_reduce_stats: the same shape and depth, other pairs.  Rows without a neighbour and rows
 *                     past n join as the identity (+0.0).  An index >= m: info[0] |= 2, the row is skipped.
 *                     workspace: vfn_icp_accumulate_workspace_bytes(n) bytes (the partials); -1 on error.
 *   vfn_nn_nearest    (csrc/vfn_nn.hip) the UNBOUNDED search, with the index: for every query i, over ALL targets j, the minimum of
 *                     (d2(j), j) in lexicographic order, d2(j) = (dx dx + dy dy) + dz dz with dx = q.x - t_j.x, ... (no transform
 *                     argument): sqdist[i] = that d2 — vfn_nn_sqdist's best[i] bit for bit — and index[i] = the LOWEST original index
 *                     that attains it.  The definition does not mention a grid and the grid changes no bit; it only bounds the work.
 *                     The grid is vfn_nn_radius's, with the same meaning of sorted_targets, perm, cell_start, box[7] (HOST memory),
 *                     nx, ny, nz, cell(), order[n] and check_finite; no radius: the cell edge h = box[6] is any normal number with
 *                     (e - o) / h <= 129 on every axis and ((VFN_ICP_GRID_CAP + 2) h)^2 finite.
 *                     One lane per query.  Per axis a = fl(fl(min(max(x, o), e) - o) / h), c = cell(x), f = a - c (exact);
 *                     s = the minimum over the three axes of min(f, max(fl(1 - f), 0)).  Ring r = the cells at Chebyshev distance
 *                     exactly r from (c_x, c_y, c_z), clipped to the grid.  The rings are visited in the order r = 0, 1, ...; after
 *                     ring r the query STOPS when rings 0..r cover the whole grid, or when
 *                       fl(r + s) >= 2^-20  and  lb >= 2^-1022  and  best < lb,   w = fl(fl(r + s) h),  lb = fl(fl(w w) (1 - 2^-20)),
 *                     best = the least d2 so far (+inf before the first target); its outputs are then written (index -1 and +inf
 *                     only when no target has d2 < +inf).  A query that has not stopped after ring max_rings (>= 0) is a LEFTOVER:
 *                     its outputs are not written, its number i goes to leftover[k], k = an integer atomicAdd of 1 on
 *                     leftover_count[0] (device memory, zero-filled by the caller; leftover has room for n entries).  The order of
 *                     the list is arbitrary and no output depends on it; its LENGTH is a function of the queries, the grid and
 *                     max_rings alone.  The argument that a stopped query has missed no target that could win or tie is in
 *                     csrc/vfn_nn.hip.
 *   vfn_nn_nearest_list  the same minimum for the count queries listed in leftover[count] (1 <= count <= n), by all m targets[m, 3] in
 *                     their ORIGINAL order, one wave per query: writes index[i] and sqdist[i] of the listed queries only.  With every
 *                     query listed this is the all-pairs search with an index.
 * ============================================================================================= */
#define VFN_ICP_GRID_CAP 128          /* cells per axis at most */
#define VFN_ICP_GRID_MARGIN_LOG2 20   /* the cell edge is at least radius (1 + 2^-20) */
int vfn_transform_points(const double* points, int64_t n, const double* transform, double* out, void* stream);
int vfn_nn_radius(const double* queries, int64_t n, const double* transform, const double* sorted_targets, const int64_t* perm,
                  int64_t m, const int32_t* cell_start, const double* box, int32_t nx, int32_t ny, int32_t nz, double radius,
                  const int64_t* order, int32_t check_finite, int64_t* index, double* sqdist, int64_t* info, void* stream);
int64_t vfn_icp_accumulate_workspace_bytes(int64_t n);
int vfn_icp_accumulate(const double* queries, int64_t n, const double* transform, const double* targets, int64_t m,
                       const int64_t* index, const double* sqdist, const double* anchor, double* sums, int64_t* info,
                       void* workspace, int64_t workspace_bytes, void* stream);
int vfn_nn_nearest(const double* queries, int64_t n, const double* sorted_targets, const int64_t* perm, int64_t m,
                   const int32_t* cell_start, const double* box, int32_t nx, int32_t ny, int32_t nz, int32_t max_rings,
                   const int64_t* order, int32_t check_finite, int64_t* index, double* sqdist, int64_t* leftover,
                   int64_t* leftover_count, int64_t* info, void* stream);
int vfn_nn_nearest_list(const double* queries, int64_t n, const double* targets, int64_t m, const int64_t* leftover, int64_t count,
                        int64_t* index, double* sqdist, void* stream);

/* =============================================================================================
 * The closest point ON a triangle mesh (csrc/vfn_proximity.hip, csrc/vfn_proximity_core.h): for every query the distance to the
 * surface, the point of the surface that attains it, and the face that point lies on.  A SPECIFICATION of ours, following the
 * closest-point queries of trimesh and Open3D as remembered; verified against neither.  Everything is float64, evaluated without
 * contraction in the association written here; no result depends on the order in which workgroups arrive; no floating-point atomics.
 * `info` as above: zero-filled by the caller and only ever OR-ed into, bit 1 = a non-finite coordinate of a query or of a vertex that
 * a face names, bit 2 = a face index outside [0, n_vertices), through which nothing is read.  1 <= n, n_vertices, n_faces < 2^31.
 *
 * THE PAIR ROUTINE  vfn_closest_on_triangle: (q, A, B, C) -> (c[3], d2)  (csrc/vfn_proximity_core.h, one text for device and host), a
 * pure function of its twelve inputs.  With dot(a, b) = (a0 b0 + a1 b1) + a2 b2, cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2,
 * a0 b1 - a1 b0), every difference, product, sum and quotient rounded once:
 *   box        lo_k = min(A_k, B_k, C_k), hi_k = max(A_k, B_k, C_k) per axis, by comparisons (lo = A; if B < lo: lo = B; if C < lo:
 *              lo = C), so that a bound is one of the inputs in its own bits.
 *   segment(P, Q)   d = Q - P, w = q - P, dd = dot(d, d), t = dot(w, d) / dd.  dd == 0 or t <= 0: P itself (its bits); otherwise
 *              t >= 1: Q itself; otherwise P + t d per component.
 *   candidates 1, 2, 3   segment(A, B), segment(B, C), segment(C, A).
 *   candidate 4     n = cross(B - A, C - A), nn = dot(n, n); only when nn > 0: s = dot(q - A, n) / nn, p = q - s n per component, and
 *              the three edge functions side(P1, P2) = dot(cross(P2 - P1, p - P1), n) for (A, B), (B, C), (C, A).  p is offered when
 *              all three are >= 0 (a foot ON an edge's line, side == 0, counts as inside; a NaN side does not).
 *   candidates 5, 6, 7   A, B, C themselves.
 *   clamp      every candidate x is replaced per component by: if not (x >= lo) then lo; then if not (x <= hi) then hi.  In exact
 *              arithmetic this changes nothing; in floating point it moves a component by a rounding error at most; a NaN component
 *              (possible only where a product of finite inputs overflowed) becomes lo.
 *   d2         of a clamped candidate x: (dx dx + dy dy) + dz dz with dx = q_x - x_x, ... — vfn_nn_sqdist's expression.
 *   result     the candidate with the least (d2, candidate number) in lexicographic order: c = that clamped candidate, d2 = its d2.
 * Candidates 5-7 are NOT in the form this routine was first drawn up in (candidates 1-4 only), which has a flaw: a segment's interior
 * a vertex is a candidate there only when some segment's t leaves (0, 1).  For a query far above a corner of the triangle, its foot
 * just inside, both adjacent segments answer with a rounded interior point and candidate 4 with a rounded foot; the true gain over
 * the corner is far below the rounding of d2, so every one of the four d2 can exceed the corner's by an ulp — and P4 below fails.
 * With the vertices offered in their own bits P4 holds by construction; tests/test_proximity_host.py records such a pair, and finds
 * more, on which candidates 1-4 alone break P4.
 * Properties (tests/test_proximity_host.py holds each):
 *   P1  finite inputs give a finite c, and no NaN anywhere in (c, d2), for degenerate triangles too (A = B, three collinear points,
 *       A = B = C: nn > 0 fails or dd == 0 answers).  d2 is finite as long as no difference q - c overflows; beyond that it is +inf,
 *       never NaN.
 *   P2  lo <= c <= hi per component, exactly.
 *   P3  d2 is exactly the point-to-point expression on c.
 *   P4  d2 <= the point-to-point expression on A, on B and on C, as a bit-exact inequality.
 *   P5  where every intermediate is exactly representable, c and d2 are the true ones.
 *
 * THE SEARCH.  For every query i, over ALL faces j whose three indices lie in [0, n_vertices), the minimum of (d2(q_i, face_j), j) in
 * lexicographic order: face[i] = the lowest face index that attains the least d2, closest[i, 3] = its c, sqdist[i] = its d2; face[i]
 * = -1, sqdist[i] = +inf and closest[i] = +inf three times when no face has d2 < +inf (a NaN query).  The definition does not mention a
 * grid and the grid changes no bit (the argument is in csrc/vfn_proximity.hip; it rests on P2, P3 and the argument of
 * csrc/vfn_nn.hip).  The grid: box[7] (HOST memory) = o[3], e[3], h as for vfn_nn_nearest, with o / e the componentwise minimum /
 * maximum over the vertices that some face names, and h, nx, ny, nz under vfn_nn_nearest's limits; cell() is vfn_nn_radius's.
 *   vfn_tri_cell_ranges  one lane per face j: tri[j, 9] = A, B, C; per axis cell_lo[j, k] = cell(lo_k), cell_hi[j, k] = cell(hi_k);
 *                     ncells[j] = the product of (cell_hi - cell_lo + 1) >= 1.  A face with an index outside [0, n_vertices):
 *                     info |= 2, tri[j] = 0, ncells[j] = 0 — no later kernel evaluates a face with ncells = 0.
 *   vfn_tri_cell_pairs   a face with 1 <= ncells[j] <= big_face_cells writes (key, j) for each of its cells, x outermost, at
 *                     offset[j] .. offset[j] + ncells[j] (offset = the exclusive prefix sums of the ncells of exactly those faces,
 *                     n_pairs their total; the caller's, as is the stable sort by key and cell_start afterwards); key as for
 *                     vfn_nn_radius.  Faces with ncells[j] > big_face_cells are LARGE: the caller lists them in ascending order.
 *                     big_face_cells changes the time only.  Tables that contradict each other: info |= 2, nothing is written.
 *   vfn_tri_nearest   one lane per query: first every face of large[n_large], then the rings of vfn_nn_nearest over
 *                     pair_face[n_pairs] (the faces of the pairs in sorted order) and cell_start[nx ny nz + 1], with ITS stop rule —
 *                     the same s, w, lb and guards, with best = the least d2 so far, large faces included — and its max_rings,
 *                     order[n], leftover[n] and leftover_count.  A face met in several cells is evaluated again or skipped; either
 *                     way the result is the same.  n_pairs = 0 (pair_face may be NULL) and n_large = 0 (large may be NULL) are valid.
 *   vfn_tri_nearest_list  the same minimum for the count queries of list[count] (1 <= count <= n) by all faces in their ORIGINAL
 *                     order, one wave per query, skipping ncells[j] = 0.  With every query listed this is the all-pairs search.
 * Both search kernels set bit 1 for a non-finite query coordinate; vfn_tri_cell_ranges for a non-finite named vertex.
 * ============================================================================================= */
int vfn_tri_cell_ranges(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, const double* box,
                        int32_t nx, int32_t ny, int32_t nz, double* tri, int32_t* cell_lo, int32_t* cell_hi, int32_t* ncells,
                        int64_t* info, void* stream);
int vfn_tri_cell_pairs(const int32_t* cell_lo, const int32_t* cell_hi, const int32_t* ncells, const int64_t* offset, int64_t n_faces,
                       int64_t big_face_cells, int32_t nx, int32_t ny, int32_t nz, int64_t n_pairs, int32_t* key, int32_t* face,
                       int64_t* info, void* stream);
int vfn_tri_nearest(const double* queries, int64_t n, const double* tri, int64_t n_faces, const int32_t* pair_face, int64_t n_pairs,
                    const int32_t* cell_start, const int64_t* large, int64_t n_large, const double* box, int32_t nx, int32_t ny,
                    int32_t nz, int32_t max_rings, const int64_t* order, int64_t* face, double* closest, double* sqdist,
                    int64_t* leftover, int64_t* leftover_count, int64_t* info, void* stream);
int vfn_tri_nearest_list(const double* queries, int64_t n, const double* tri, const int32_t* ncells, int64_t n_faces,
                         const int64_t* list, int64_t count, int64_t* face, double* closest, double* sqdist, int64_t* info,
                         void* stream);

/* =============================================================================================
 * Scoring rendered views (csrc/vfn_image.hip): the image half of evaluation/methods.py:549-610 (metrics) — utils/utils.py:235-245
 * (get_psnr), :248-289 (get_ssim), :312-325 (get_l1_cm) and the save_rgb -> PNG -> load_rgb round trip (:73-108).  A float64
 * SPECIFICATION of the reference's formulas (the reference evaluates them in float32).  Everything is float64, evaluated without
 * contraction in the association written here; no result depends on the order in which workgroups arrive; no floating-point atomics.
 * `info` as above: zero-filled by the caller and only ever OR-ed into, bit 1 = a non-finite value, bit 4 = a value outside the range of
 * a byte.  Images are V views of H x W x C values, interleaved, row-major.  Limits: 1 <= V, 1 <= H, W < 2^15, C in {1, 3},
 * V H W C < 2^31; anything else is refused before any launch.
 *   vfn_image_quantize8  u[i] = trunc(double(x[i]) 255.0) for x[n] float32, 1 <= n < 2^31.  The product is exact (24 bits x 8 bits), so
 *                     this is numpy's (x.astype(float64) * 255).astype(uint8) — what save_rgb writes for a float64 image — wherever
 *                     that cast is defined.  Where it is not, the value is refused instead of wrapped: x not finite: info[0] |= 1;
 *                     x < 0 or double(x) 255.0 >= 256: info[0] |= 4; u[i] = 0 in both cases.  (-0.0 is 0.)
 *   vfn_image_scores  pred and target are uint8 (p = double(u) / 255.0, the division rounded once) or float32 (p = double(x)), chosen
 *                     by pred_u8 / target_u8.  Writes sums[V, 3], both sums over all H W C elements of view v:
 *                       sums[v][0] = sum (p - t)^2        (the difference rounded once, the square once)
 *                       sums[v][1] = sum ssim(y, x, c)    (written 0 when want_ssim == 0)
 *                       sums[v][2] = 0                    (reserved)
 *                     ssim at (y, x, c), window k = 11, zero padding (a term outside the image is +0.0, the divisor always 121):
 *                     for each a in {p, t, p p, t t, p t} (each product rounded once, per element)
 *                       r_a[y'][x] = a[y'][x-5] + a[y'][x-4] + ... + a[y'][x+5]        added serially from the left, the first term as it is
 *                       S_a        = r_a[y-5][x] + r_a[y-4][x] + ... + r_a[y+5][x]     added serially from the top, the first term as it is
 *                       m_a        = S_a / 121.0
 *                     mu1 = m_p, mu2 = m_t, s1 = m_pp - mu1 mu1, s2 = m_tt - mu2 mu2, s12 = m_pt - mu1 mu2,
 *                       ssim = ((2 (mu1 mu2) + C1) (2 s12 + C2)) / (((mu1 mu1 + mu2 mu2) + C1) ((s1 + s2) + C2))
 *                     (get_ssim's defaults: C1 = 1e-4, C2 = 9e-4).  With p == t every element is exactly 1.0.  No running window.
 *                     A non-finite float32 element: info[0] |= 1.
 *   vfn_image_abs_err a[V, H, W], b[V, H, W] float32: sums[v] = sum |double(a) s - double(b) s|, each product rounded once; s = 100 is
 *                     get_l1_cm's sum.  A kernel of its own over the tiles of a C = 1 image; the sums are joined as below.
 *   The sums go along THE FIXED TREE (above, after vfn_reduce_stats) without a lane tree.  A workgroup owns a tile of VFN_IMAGE_TILE x
 *   VFN_IMAGE_TILE = 16 x 16 pixels; tile (tile_y, tile_x) starts at pixel (16 tile_y, 16 tile_x); lane l = 16 ly + lx owns pixel
 *   (16 tile_y + ly, 16 tile_x + lx) and adds its C elements serially in ascending c, the first as it is; a lane outside the image holds
 *   +0.0.  The block tree joins the 256 lane values into one partial per tile, in (view, tile_y, tile_x) order; the second level runs
 *   once per view over that view's P = ceil(H / 16) ceil(W / 16) partials.  The bits are a function of (V, H, W, C) and the data alone.
 *   workspace: vfn_image_scores_workspace_bytes(V, H, W, C) bytes (vfn_image_abs_err: C = 1); answers on the host, -1 on error.
 * ============================================================================================= */
#define VFN_IMAGE_TILE 16
int vfn_image_quantize8(const float* x, int64_t n, uint8_t* u, int64_t* info, void* stream);
int64_t vfn_image_scores_workspace_bytes(int64_t V, int64_t H, int64_t W, int64_t C);
int vfn_image_scores(const void* pred, int32_t pred_u8, const void* target, int32_t target_u8, int64_t V, int64_t H, int64_t W, int64_t C,
                     int32_t want_ssim, double c1, double c2, double* sums, int64_t* info, void* workspace, int64_t workspace_bytes,
                     void* stream);
int vfn_image_abs_err(const float* a, const float* b, int64_t V, int64_t H, int64_t W, double scale, double* sums, int64_t* info,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* =============================================================================================
 * Fusing depth maps into a mesh (csrc/vfn_tsdf.hip): the stage of evaluation/methods.py:613-665 (tsdf_mesh) between the rendered depth
 * maps and the mesh that metrics_3d scores, with the semantics of a uniform TSDF volume — projective integration with a running mean,
 * classic marching cubes on the zero level set.  Two deliberate differences: the volume is DENSE over a box the caller gives (not
 * hashed 16^3 blocks opened near back-projected points, so a voxel in free space in front of a surface collects tsdf = 1 observations
 * that a hashed volume would never have allocated; the zero crossing lies inside the truncation band either way — the block-sparse
 * volume of the next section opens blocks of 8^3 voxels of this same lattice near the points), and colour is
 * optional: a volume without one keeps its entry points and its bits, a volume with one adds colour[nx, ny, nz, 3] (below).
 * Volume: tsdf[nx, ny, nz] and weight[nx, ny, nz], float32, C order (k fastest), zero-filled by the caller before the first view;
 * voxel (i, j, k) has its centre at origin + (index + 0.5) voxel_length.  nx ny nz < 2^31, voxel_length > 0, sdf_trunc > 0.
 *   vfn_tsdf_integrate  depth[V, H, W] (float32 metres, 0 = no measurement), intrinsics[V, 4] = fx fy cx cy, extrinsics[V, 12] = the
 *                     world -> camera rows e00 .. e23.  Per voxel and view, in float32, every operation rounded once in the
 *                     association written (no contraction, correctly rounded / and sqrtf):
 *                       x = ox + ((float)i + 0.5f) vl                                   (y, z alike)
 *                       xc = ((e00 x + e01 y) + e02 z) + e03                            (yc, zc alike)
 *                       skip unless zc > 0
 *                       u = floorf(((xc fx) / zc + cx) + 0.5f);  v = floorf(((yc fy) / zc + cy) + 0.5f)
 *                       skip unless 0 <= u < W and 0 <= v < H
 *                       d = depth[v, u];  skip unless d > 0
 *                       a = (u - cx) / fx;  b = (v - cy) / fy;  m = sqrtf((1.0f + a a) + b b)
 *                       sdf = (d - zc) m;  skip unless sdf > -sdf_trunc
 *                       t = fminf(1.0f, sdf / sdf_trunc)
 *                       tsdf = (tsdf weight + t) / (weight + 1.0f);  weight = weight + 1.0f
 *                     The views of one call are applied in index order per voxel, rounded to float32 after each: the bits of V
 *                     single-view calls in that order.  The volume is read and written once per call, whatever V is.  A workgroup
 *                     may skip a view that provably touches none of its voxels; skipping never changes a bit.
 *   vfn_tsdf_count    cells (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, in C order; corners in the order of vfn_mesh_tables
 *                     ((0,0,0) (0,1,0) (1,1,0) (1,0,0) (0,0,1) (0,1,1) (1,1,1) (1,0,1)).  A cell with any corner at weight == 0 counts
 *                     0; case bit q is set iff tsdf_q < 0 (exactly 0 is outside); counts[cell] = triangles of the classic table's
 *                     row, offsets = their inclusive scan, info[0] = triangles T.  counts / offsets: (nx-1)(ny-1)(nz-1) int32; the
 *                     scan workspace is vfn_mesh_scan_workspace_bytes(cells).
 *   vfn_tsdf_emit     tri_verts[3 T, 3] (double), triangles in the table row's order at slot 3 (offsets[cell] - counts[cell] + t) +
 *                     corner: the layout vfn_mesh_dedup / vfn_mesh_number consume.  A vertex is computed from its edge alone — L the
 *                     endpoint with the lower lattice index, U the other (one step along one axis), f = (double)|tsdf|:
 *                       position[c] = (double)origin[c] + ((double)index_L[c] + 0.5) (double)vl       on all three axes
 *                       position[axis] = position[axis] + (f_L / (f_L + f_U)) (double)vl
 *                     in float64 without contraction, so the cells around an edge emit identical bits and the positional merge joins
 *                     them; vertices that coincide at a corner whose tsdf is exactly 0 merge too, degenerate faces are kept.
 * Colour (evaluation/methods.py:626: TSDFVolumeColorType.RGB8, convert_rgb_to_intensity=False): colour[nx, ny, nz, 3], float32, C order,
 * in byte units (0 .. 255), zero-filled by the caller before the first view.
 *   vfn_tsdf_integrate_rgb  vfn_tsdf_integrate with colour and rgb[V, H, W, 3] (uint8).  Per voxel and view the tests and the tsdf /
 *                     weight update are exactly those above; where that update is applied, each channel c is updated with the weight
 *                     BEFORE its increment, in float32, every operation rounded once in the association written, no contraction:
 *                       colour_c = (colour_c weight + (float)rgb[v, u, c]) / (weight + 1.0f)
 *                     with (v, u) the pixel the depth was read from.  Views in index order per voxel (the bits of V single-view
 *                     calls), the volume read and written once per call; tsdf and weight come out bit-identical to
 *                     vfn_tsdf_integrate on the same inputs.
 *   vfn_tsdf_emit_colours  counts / offsets from vfn_tsdf_count; tri_cols[3 T, 3] (double) in the slot layout of vfn_tsdf_emit.  For a
 *                     cut edge with endpoints L, U and f = (double)|tsdf| as in the position formula, in float64 without contraction:
 *                       r = f_L / (f_L + f_U)
 *                       col[c] = ((1.0 - r) (double)colour_L[c] + r (double)colour_U[c]) / 255.0
 *                     (r = 0 gives colour_L / 255 exactly, r = 1 gives colour_U / 255 exactly).
 *   vfn_tsdf_vertex_colours  ids[S] (the slot -> vertex numbering of vfn_mesh_number), tri_cols[S, 3] -> colours[n_vertices, 3] (double): a
 *                     vertex takes the colour of the slot at which it first appears, the LOWEST slot carrying its id — the slot whose
 *                     position bits vfn_mesh_dedup keeps.  (Two different edges can round to one position with colours that differ in
 *                     the last bit; equal colour bits on all slots of a vertex are not relied on.)  first[n_vertices] (int32) is
 *                     workspace: the lowest slot per vertex, found with an integer atomicMin per slot.
 * Limits: 3 T < 2^31.  No floating-point atomics; one integer atomicMin per slot in vfn_tsdf_vertex_colours only.
 * ============================================================================================= */
int vfn_tsdf_integrate(float* tsdf, float* weight, int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz,
                       float voxel_length, float sdf_trunc, const float* depth, int32_t height, int32_t width,
                       const float* intrinsics, const float* extrinsics, int32_t n_views, void* stream);
int vfn_tsdf_count(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, int32_t* counts, int32_t* offsets,
                   int64_t* info, void* scan_ws, int64_t scan_ws_bytes, void* stream);
int vfn_tsdf_emit(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz,
                  float voxel_length, const int32_t* counts, const int32_t* offsets, double* tri_verts, void* stream);
int vfn_tsdf_integrate_rgb(float* tsdf, float* weight, float* colour, int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz,
                           float voxel_length, float sdf_trunc, const float* depth, const uint8_t* rgb, int32_t height, int32_t width,
                           const float* intrinsics, const float* extrinsics, int32_t n_views, void* stream);
int vfn_tsdf_emit_colours(const float* tsdf, const float* weight, const float* colour, int32_t nx, int32_t ny, int32_t nz,
                          const int32_t* counts, const int32_t* offsets, double* tri_cols, void* stream);
int vfn_tsdf_vertex_colours(const int64_t* ids, int64_t n_slots, const double* tri_cols, int32_t* first, int64_t n_vertices,
                            double* colours, void* stream);

/* =============================================================================================
 * A block-sparse TSDF volume (csrc/vfn_tsdf.hip, after the dense entry points): the SAME voxel lattice as above — origin, dims = (nx, ny,
 * nz), voxel_length as float32, voxel (i, j, k) centred at origin + ((float)index + 0.5f) vl with the GLOBAL index — held as blocks of
 * 8^3 voxels that exist only near the back-projected depth points.  Every voxel it holds carries the bits of the dense volume over the
 * same lattice; dims are not bound by 2^31 voxels.  Limits: each dim <= 2^24; the block lattice nb = ceil(dims / 8) has nbx nby nbz <
 * 2^31; n_blocks 512 < 2^31.
 * Storage: block_of[nbx, nby, nbz] int32 (-1: absent), block_coords[n_blocks, 3] int32, tsdf / weight [n_blocks, 8, 8, 8] float32 and
 * colour [n_blocks, 8, 8, 8, 3] float32 (byte units), C order, 16-B aligned, zero-filled when a block is opened.  Block ids are given by
 * the caller (vf_nerf_amd/tsdf.py: in order of allocation call, inside a call in ascending C order of the block lattice, from
 * torch.nonzero of the marks — no atomics decide a number) and never change.
 *   vfn_tsdf_sparse_mark  one lane per pixel of depth[V, H, W]; cameras[V, 17] (double) = C[12], fx, fy, cx, cy, q with C the first three
 *                     rows of the float64 inverse of the 4x4 whose first three rows are the float32 extrinsic rows promoted (the matrix
 *                     the integration uses), fx fy cx cy the float32 intrinsics promoted and q = sqrt(1 / (fx fx) + 1 / (fy fy)).  With
 *                     o, vl, tr the float32 origin, voxel_length and sdf_trunc promoted, all in float64, every operation rounded once in
 *                     the association written, no contraction:
 *                       d = (double)depth[v, u];  skip unless d > 0
 *                       a = ((double)u - cx) / fx;  b = ((double)v - cy) / fy
 *                       P[c] = ((C[c][0] (a d) + C[c][1] (b d)) + C[c][2] d) + C[c][3]
 *                       r = (tr + (0.5 (d + tr)) q) + 2.0 vl
 *                       lo[c] = floor(((P[c] - r) - o[c]) / (8.0 vl));  hi[c] = floor(((P[c] + r) - o[c]) / (8.0 vl))
 *                       skip unless hi[c] >= 0 and lo[c] <= nb[c] - 1 on every axis (a NaN skips);  clamp both to [0, nb[c] - 1]
 *                       marks[bi, bj, bk] = 1 for lo <= (bi, bj, bk) <= hi
 *                     marks[nbx, nby, nbz] (uint8) is zeroed by the caller; the store is a plain byte store of the constant 1 (lanes that
 *                     race store the same value; a lane may read the byte and skip the store).  Why this radius: DESIGN 6p.
 *   vfn_tsdf_sparse_integrate / _rgb  all V views into EVERY block of block_coords, one workgroup of 128 lanes per block, a lane owning 4
 *                     consecutive k voxels.  Per voxel and view the arithmetic is vfn_tsdf_integrate's (vfn_tsdf_integrate_rgb's) — the
 *                     same device function — with x, y, z from the global index 8 block_coords + local; views in index order; a view is
 *                     skipped for a block only by the dense kernel's exact brick test.  A voxel whose global index is >= dims is never
 *                     updated and keeps weight == 0.  A block is read and written once per call, whatever V is.
 *   vfn_tsdf_sparse_count / _emit / _emit_colours  the extraction of vfn_tsdf_count / _emit / _emit_colours over n_blocks 512 positions:
 *                     position p is block p >> 9 and local cell ((p >> 6) & 7, (p >> 3) & 7, p & 7), the global cell g = 8 block_coords
 *                     + local.  A cell with g[c] + 1 >= dims[c] on any axis counts 0; a corner comes from this block or from the
 *                     neighbour block_of names, and an absent neighbour voids the cell like a corner with weight == 0.  Case, triangle
 *                     order, vertex position (with the global lattice index) and colour are the dense formulas: a vertex has the dense
 *                     mesh's bits, and vfn_mesh_dedup joins it across blocks.  counts / offsets: n_blocks 512 int32.
 * ============================================================================================= */
int vfn_tsdf_sparse_mark(uint8_t* marks, int32_t nbx, int32_t nby, int32_t nbz, float ox, float oy, float oz, float voxel_length,
                         float sdf_trunc, const float* depth, int32_t height, int32_t width, const double* cameras, int32_t n_views,
                         void* stream);
int vfn_tsdf_sparse_integrate(float* tsdf, float* weight, const int32_t* block_coords, int32_t n_blocks, int32_t nx, int32_t ny,
                              int32_t nz, float ox, float oy, float oz, float voxel_length, float sdf_trunc, const float* depth,
                              int32_t height, int32_t width, const float* intrinsics, const float* extrinsics, int32_t n_views,
                              void* stream);
int vfn_tsdf_sparse_integrate_rgb(float* tsdf, float* weight, float* colour, const int32_t* block_coords, int32_t n_blocks, int32_t nx,
                                  int32_t ny, int32_t nz, float ox, float oy, float oz, float voxel_length, float sdf_trunc,
                                  const float* depth, const uint8_t* rgb, int32_t height, int32_t width, const float* intrinsics,
                                  const float* extrinsics, int32_t n_views, void* stream);
int vfn_tsdf_sparse_count(const float* tsdf, const float* weight, const int32_t* block_of, const int32_t* block_coords, int32_t n_blocks,
                          int32_t nx, int32_t ny, int32_t nz, int32_t* counts, int32_t* offsets, int64_t* info, void* scan_ws,
                          int64_t scan_ws_bytes, void* stream);
int vfn_tsdf_sparse_emit(const float* tsdf, const float* weight, const int32_t* block_of, const int32_t* block_coords, int32_t n_blocks,
                         int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float voxel_length, const int32_t* counts,
                         const int32_t* offsets, double* tri_verts, void* stream);
int vfn_tsdf_sparse_emit_colours(const float* tsdf, const float* weight, const float* colour, const int32_t* block_of,
                                 const int32_t* block_coords, int32_t n_blocks, int32_t nx, int32_t ny, int32_t nz,
                                 const int32_t* counts, const int32_t* offsets, double* tri_cols, void* stream);

/* =============================================================================================
 * Rasterising a mesh's depth, and Laplacian smoothing (csrc/vfn_raster.hip): what evaluation/methods.py:33-72 (refuse: the mesh's depth
 * from every dataset view by an OpenGL renderer, faces not culled, re-fused with depth_scale 1 / depth_trunc 5) and :686-691
 * (filter_smooth_laplacian, 10 iterations) need on top of the TSDF volume.  Neither renderer nor filter is reproduced bit for bit (no
 * fixed arithmetic is published for either): this is a SPECIFICATION, restated in tests/raster_restatement.py.
 *   vfn_raster_depth  vertices[n, 3] (double, world), faces[m, 3] (int64, 0-based), intrinsics[V, 4] = fx fy cx cy, extrinsics[V, 12] =
 *                     the world -> camera rows e00 .. e23 (float32; the camera looks along +z, x right, y down), near, far,
 *                     pixel_centre c (float32).  Writes depth[V, H, W] (float32): the z-depth of the nearest surface, 0 where there
 *                     is none.  All arithmetic float64 with the float32 inputs promoted, every operation rounded once in the
 *                     association written, no contraction, correctly rounded /.  Per view and face (q = 0, 1, 2 its vertices):
 *                       P_q.x = ((e00 X + e01 Y) + e02 Z) + e03                                  (y, z alike)
 *                       skip the face if all three P_q.z < near, or all three P_q.z > far
 *                       n0 = P1 x P2,  n1 = P2 x P0,  n2 = P0 x P1          (a x b).x = a.y b.z - a.z b.y, cyclic
 *                       D = (P0.x n0.x + P0.y n0.y) + P0.z n0.z;  skip the face if D == 0 or D is not finite
 *                       candidate pixels — all three P_q.z >= near:  px_q = (P_q.x fx) / P_q.z + cx,  py_q alike;
 *                           u from max(0, ceil(min px - c) - 1) to min(W - 1, floor(max px - c) + 1), v alike (an empty range
 *                           skips the face); otherwise (the face straddles the near plane): every pixel of the view
 *                       per candidate pixel (u, v):
 *                         dx = (((double)u + c) - cx) / fx;  dy = (((double)v + c) - cy) / fy
 *                         e_i = (n_i.x dx + n_i.y dy) + n_i.z        i = 0, 1, 2 — evaluated directly, never incrementally
 *                         s = (e0 + e1) + e2
 *                         covered iff s != 0 and, with sigma = sign(D), sigma e_i >= 0 for all three i (edges inclusive, no culling)
 *                         z = D / s;  kept iff near <= z <= far;  candidate value (float)z
 *                       depth[v, u] = the minimum candidate value over all faces, 0 if there is none
 *                     (ray / triangle intersection as homogeneous edge functions: for the ray (dx, dy, 1), z is the z-depth.  A face
 *                     through the camera plane needs no clipping; the two faces of an edge get exactly negated n_i, so a closed
 *                     surface has no holes without a fill rule; the minimum commutes, so no bit depends on face order or schedule.)
 *                     depth is filled and finished inside the call.  info[4] (int64, zero-filled by the caller, only added to / OR-ed
 *                     into): info[0] bit 1 = a non-finite vertex coordinate, bit 2 = a face index outside [0, n) — such a face is
 *                     not drawn and nothing is read through its indices; with either bit set depth is meaningless.  info[1] =
 *                     fragments (kept candidates), info[2] = atomics sent, info[3] = (face, view) pairs walked by a whole wave.
 *                     Limits: 0 < near < far finite, c finite, H, W >= 1, V H W < 2^31, n, m < 2^31.  Every argument check answers
 *                     before any launch.
 *   vfn_smooth_laplacian_step  one Jacobi step src[n, 3] -> dst[n, 3] (double, two different arrays) over a CSR adjacency:
 *                     row_start[n + 1], neighbours[row_start[n]] (int64), a vertex's neighbours in ascending order, each once:
 *                       s = v[nb_0];  s = s + v[nb_1];  ...                  per component, in the row's order
 *                       new = v + lam (s / (double)count - v)
 *                     a vertex without neighbours is copied.  info[0] bit 2 = a row or a neighbour outside its range (that vertex is
 *                     copied).  float64 without contraction, no atomics.
 * ============================================================================================= */
int vfn_raster_depth(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, const float* intrinsics,
                     const float* extrinsics, int32_t n_views, int32_t height, int32_t width, float near, float far, float pixel_centre,
                     float* depth, int64_t* info, void* stream);
int vfn_smooth_laplacian_step(const double* src, double* dst, int64_t n_vertices, const int64_t* row_start, const int64_t* neighbours,
                              int64_t n_neighbours, double lam, int64_t* info, void* stream);

/* =============================================================================================
 * Normals of a triangle mesh and the dots of normal consistency (csrc/vfn_normals.hip): what the reference leaves to Open3D's
 * compute_vertex_normals() before it writes tsdf.ply (evaluation/methods.py:664-665), and the third score beside chamfer distance and
 * F-score.  A SPECIFICATION: area-weighted vertex normals are Open3D's compute_vertex_normals() as remembered, not verified against
 * Open3D, and Open3D's sums have no fixed order.  Everything is float64, evaluated without contraction in the association written
 * here, with no floating-point atomics: no bit depends on the schedule.  Indices are int64.  info[0] (int64, zero-filled by the caller,
 * only OR-ed into): bit 1 = a non-finite coordinate or normal was read, bit 2 = an index outside its range — nothing is read through
 * such an index and that row's output is the fallback —, bit 4 = a length that overflowed (finite inputs, a non-finite cross product or
 * a non-finite r below).  Limits: 0 <= n, m < 2^31 (a count of 0 launches nothing).  Every argument check answers before any launch.
 *   unit(c, fallback):  s = c.x c.x;  s = s + c.y c.y;  s = s + c.z c.z;  r = sqrt(s) (correctly rounded);
 *                     r > 0 and finite: (c.x / r, c.y / r, c.z / r), three divisions; otherwise `fallback`, and info bit 4 if r is
 *                     not finite.
 *   vfn_face_normals  reads vertices[n, 3], faces[m, 3]; one lane per face: a = v1 - v0, b = v2 - v0,
 *                       c = (a.y b.z - a.z b.y,  a.z b.x - a.x b.z,  a.x b.y - a.y b.x)      two products and one subtraction each
 *                     normalise = 0: out[m, 3] = c (its length is twice the area; bit 4 if it is not finite although the coordinates
 *                     are); normalise = 1: out = unit(c, (0, 0, 0)).  A face with an index outside [0, n): bit 2, out = (0, 0, 0).
 *   vfn_vertex_normals  reads face_normals[m, 3] (the UNNORMALISED ones) and a CSR of every vertex's faces: row_start[n + 1],
 *                     incident[row_start[n]], a vertex's faces ascending, each once.  One lane per vertex:
 *                       s = fn[f_0];  s = s + fn[f_1];  ...                     per component, in the row's order
 *                       out[n, 3] = unit(s, (0, 0, 1))
 *                     — area weighting.  A vertex without faces gets (0, 0, 1).  A row outside [0, row_start[n]] (read on the device)
 *                     or a face outside [0, m): bit 2, (0, 0, 1).  A long row is slow (one lane walks it) and stays correct.
 *   vfn_normal_dots   reads qn[n, 3], tn[m, 3], index[n]; with j = index[i]:
 *                       d = qn.x tn[j].x;  d = d + qn.y tn[j].y;  d = d + qn.z tn[j].z;  out[i] = fabs(d)
 *                     j outside [0, m): bit 2, out[i] = 0.
 * ============================================================================================= */
int vfn_face_normals(const double* vertices, int64_t n, const int64_t* faces, int64_t m, int32_t normalise, double* out, int64_t* info,
                     void* stream);
int vfn_vertex_normals(const double* face_normals, int64_t m, const int64_t* row_start, const int64_t* incident, int64_t n, double* out,
                       int64_t* info, void* stream);
int vfn_normal_dots(const double* qn, int64_t n, const double* tn, int64_t m, const int64_t* index, double* out, int64_t* info, void* stream);

/* =============================================================================================
 * Voxel down-sampling of a point set (csrc/vfn_voxel.hip; vf_nerf_amd/voxel.py, metrics3d.voxel_down_sample): the first step of the
 * evaluate_3d_reconstruction protocol the reference's metrics_3d calls — both clouds are down-sampled before they are registered and
 * before precision and recall are counted, so that every occupied voxel votes once.  A SPECIFICATION of ours that imitates Open3D's
 * voxel_down_sample AS REMEMBERED: neither Open3D nor that package is available to compare against, and Open3D's hash map fixes no
 * order of summation; ours does.  Everything is float64, evaluated without contraction in the association written here, with no
 * floating-point atomics: no bit depends on the schedule.  Keys, tables and counts are int64.
 *   The frame (host arithmetic, Python floats): h = voxel_size, finite and > 0 with a normal square;
 *                       origin_k = min_k(points) - 0.5 h             (Open3D's voxel_min_bound)
 *                       dims_k   = floor((max_k(points) - origin_k) / h) + 1 <= 2^VFN_VOXEL_AXIS_BITS
 *   vfn_voxel_keys    reads points[n, 3] and the HOST values origin[3], h; one lane per point:
 *                       c_k = floor((p_k - origin_k) / h)              a subtraction and a true division, in exactly this expression
 *                       keys[i] = (c_0 << 42) | (c_1 << 21) | c_2      as int64
 *                     A non-finite coordinate: info bit 1, keys[i] = -1.  A c_k outside [0, 2^21) (NaN included; only an origin that is
 *                     not the box's can do that): info bit 2, keys[i] = -1.  No key indexes memory in this kernel.
 *   Order and numbering (the caller's, by a STABLE ascending sort of the keys): a voxel is a maximal run of equal keys; voxels are
 *                     numbered in ascending key — lexicographic (c_0, c_1, c_2) —; inside a voxel the points stand in ascending original
 *                     index; start[V + 1] (int64) holds every voxel's first sorted position and n.
 *   vfn_voxel_means   reads sorted_values[n, channels] (the rows gathered into sorted order, 1 <= channels <= 9) and start[n_voxels + 1];
 *                     one lane per voxel, per channel:
 *                       S = x_b;  S = S + x_(b+1);  ...  S = S + x_(e-1)       b = start[v], e = start[v + 1]: ascending position
 *                       means[v, c] = S / (double)(e - b)
 *                     The sum STARTS FROM THE FIRST ELEMENT, not from +0.0: a voxel holding one -0.0 keeps it.  The table is not
 *                     trusted: a segment that is empty, decreasing or outside [0, n] gets NaN in its row and info bit 2, and nothing is
 *                     read through it.  A voxel holding every point is walked by one lane: slow, and correct.
 * info[0] (int64, zero-filled by the caller, only OR-ed into).  Limits: 1 <= n < 2^31, 1 <= n_voxels <= n.  Every argument check
 * answers before any launch.
 * ============================================================================================= */
#define VFN_VOXEL_AXIS_BITS 21        /* a voxel index per axis lies in [0, 2^21): three of them fill 63 bits of an int64 key */
#define VFN_VOXEL_MAX_CHANNELS 9      /* points, normals and colours of one cloud in one call */
int vfn_voxel_keys(const double* points, int64_t n, const double* origin, double voxel_size, int64_t* keys, int64_t* info, void* stream);
int vfn_voxel_means(const double* sorted_values, int64_t n, int32_t channels, const int64_t* start, int64_t n_voxels, double* means,
                    int64_t* info, void* stream);

/* =============================================================================================
 * Connected components of a triangle mesh (csrc/vfn_cc.hip, csrc/vfn_forest_core.h; vf_nerf_amd/meshops.py: connected_components,
 * filter_components): what a fused mesh consists of, so that its small detached pieces can be culled before it is scored.  A
 * SPECIFICATION of ours that follows Open3D's cluster_connected_triangles and trimesh's split AS REMEMBERED: neither is available to
 * compare against, and neither fixes a numbering of the components or an order of summation; ours does.  Labels, counts and tables
 * are int64, the forest int32, areas float64 evaluated without contraction in the association written here, with no floating-point
 * atomics.  The forest's intermediate states depend on the schedule; no output does.
 *   Nodes and connectivity.  The nodes are the faces 0 .. m-1 of faces[m, 3] over n vertices.
 *                     "edge":   two faces are connected when they share an undirected edge {a, b}, a != b, among their corner pairs
 *                               (0,1), (1,2), (2,0).  A corner pair with a == b is no edge.  An edge shared by three or more faces
 *                               connects all of them.
 *                     "vertex": two faces are connected when they name a common vertex.
 *                     A component is a class of the transitive closure.
 *   Labels.           The ROOT of a component is its lowest face index.  Components are numbered 0 .. K-1 in ascending root;
 *                     first_face[K] holds the roots.  face_label[m] is the number of the face's component.  vertex_label[n] is the
 *                     LOWEST label among the faces that name the vertex (in "vertex" mode they all carry one label); -1 for a vertex
 *                     that no face names.  face_count[K] is exact.
 *   Areas.            area[K]: the vfn_tri_areas values of the component's faces in ascending face index, x_0 .. x_(c-1), added by
 *                     vfn_cc_segment_sums' rule below.
 *   The items (the caller's, torch plumbing).  "edge": the 3m corner pairs, all pairs (0,1) in face order, then all (1,2), then all
 *                     (2,0), key = min(a, b) * n + max(a, b) (-1 where a == b), node = the face, sorted ascending by key with a
 *                     STABLE sort.  "vertex": the incidences (vertex, face), each once, ascending by vertex then face, key = the
 *                     vertex, node = the face.  Faces that hold one key stand next to each other: uniting neighbours unites them all.
 *   vfn_cc_union_runs reads keys[n_items] (sorted), nodes[n_items]; updates parent[n_nodes] (int32), which the CALLER fills with the
 *                     identity.  One lane per item i >= 1: where keys[i] == keys[i-1] >= 0, the trees of nodes[i-1] and nodes[i] are
 *                     united — a concurrent union-find (csrc/vfn_forest_core.h): parent[x] <= x at all times; only a root is ever hooked,
 *                     by a compare-and-swap parent[a]: a -> b with b < a both found as roots, the finds repeated when it fails; path
 *                     halving by compare-and-swap.  After the launch two nodes are in one tree exactly when a chain of united pairs
 *                     joins them, and every tree's root is its lowest node — whatever the schedule.  A node outside [0, n_nodes):
 *                     info bit 2, the pair is not followed.  A parent outside [0, its node] (a forest that is not ours): info bit 2.
 *   vfn_cc_flatten    reads parent[n_nodes] AFTER the unions (another launch), writes root[n_nodes] (int64): where v's parent chain
 *                     ends.  A parent outside [0, its node]: info bit 2, root[v] = -1, the chain is dropped there.
 *   vfn_cc_segment_sums  reads sorted_values[n] and start[n_segments + 1]; one WAVE of 64 lanes per segment [b, e) = [start[v], start[v + 1]):
 *                       s_t = x_(b+t);  s_t = s_t + x_(b+t+64);  s_t = s_t + x_(b+t+128);  ...      lane t, serially, from its FIRST element
 *                       s_t = +0.0                                                               for a lane without elements
 *                       s_t = s_t + s_(t+32) for t < 32;  then s_t = s_t + s_(t+16) for t < 16;  then 8, 4, 2, 1;   sums[v] = s_0
 *                     — a segment of 2 x 10^6 values is 31 250 additions deep per lane, not one lane's loop.  (A lone -0.0 comes out
 *                     as +0.0: lane 0 adds lane 32's +0.0.)  The table is not trusted: a segment that is empty, decreasing or
 *                     outside [0, n] gets NaN and info bit 2, and nothing is read through it.
 * info[0] (int64, zero-filled by the caller, only OR-ed into).  Limits: 1 <= n_nodes < 2^31, 1 <= n_items < 3 * 2^31, 1 <= n < 2^31,
 * 1 <= n_segments <= n.  Every argument check answers before any launch.
 * ============================================================================================= */
int vfn_cc_union_runs(const int64_t* keys, const int64_t* nodes, int64_t n_items, int32_t* parent, int64_t n_nodes, int64_t* info,
                      void* stream);
int vfn_cc_flatten(const int32_t* parent, int64_t n_nodes, int64_t* root, int64_t* info, void* stream);
int vfn_cc_segment_sums(const double* sorted_values, int64_t n, const int64_t* start, int64_t n_segments, double* sums, int64_t* info,
                        void* stream);

/* =============================================================================================
 * Orientation of a triangle mesh (csrc/vfn_orient.hip, csrc/vfn_forest_core.h; vf_nerf_amd/meshops.py: orientation, orient,
 * inconsistent_edges): the faces rewound so that two faces that share a manifold edge traverse it in opposite directions — what the
 * contrastive marching-cubes mesh, whose cells choose their sides locally, does not give.  A SPECIFICATION of ours, not verified against
 * trimesh's fix_normals or Open3D's orient_triangles: neither is available to compare against, and neither fixes which face of a piece
 * keeps its winding; ours does.  The connected-components union-find with one more bit per node: labels, counts and tables are int64,
 * the forest int32, parities and directions uint8, votes float64 evaluated without contraction in the association written here, with
 * no floating-point atomics.  The forest's intermediate states depend on the schedule; no output does.
 *   The items (the caller's, torch plumbing).  The 3m half-edges of faces[m, 3] exactly as the "edge" items of the connected components
 *                     above: all corner pairs (0,1) in face order, then all (1,2), then all (2,0); for the half-edge a -> b
 *                     key = min(a, b) * n + max(a, b) (-1 where a == b), node = the face, and a direction byte dir = (a < b); sorted
 *                     ascending by key with a STABLE sort.
 *   Manifold edge.    A run of equal keys >= 0 of length EXACTLY two whose two items belong to different faces.  A run of length 1
 *                     (boundary), a run of length 3 or more (non-manifold), a corner pair with a == b (key -1) and a run of two items of
 *                     one face impose nothing and connect nothing.
 *   Constraint.       flip[f] says whether face f is rewound.  A manifold edge between f and g requires
 *                       flip[f] ^ flip[g] == (dir_f == dir_g)
 *                     — consistent neighbours traverse a shared edge in opposite directions.
 *   Components.       The classes of the faces under manifold edges (in general finer than the "edge" components above).  The ROOT of a
 *                     component is its lowest face index, components are numbered 0 .. K-1 in ascending root; first_face[K],
 *                     face_label[m] and face_count[K] as above.
 *   Orientable.       A component is orientable iff all its constraints can hold together; parity[f], the flip of f relative to its
 *                     component's root face, is then unique.  A component that is not is reported (orientable[c] = 0), has parity 0 on
 *                     all its faces, takes no part in the vote below, and its faces come out unchanged.
 *   The sign of a component (the caller's `reference`): flip[f] = parity[f] ^ sign[face_label[f]], sign = 0 where not orientable.
 *                     "first":      sign = 0, the root face keeps its winding.
 *                     "majority":   sign = 1 iff 2 * (faces of the component with parity 1) > face_count: the sign that flips fewer
 *                                   faces, integers only; on a tie the root keeps its winding.
 *                     "volume" / "viewpoints": every face casts a vote t (vfn_orient_votes), a component's votes in ascending face
 *                                   index are added by vfn_cc_segment_sums' rule, sign = 1 iff the sum is < 0 (a sum of 0, a NaN and a
 *                                   component of one face follow the same rule).  "volume" is meaningful for closed pieces only: the
 *                                   sum is six times the signed volume a closed piece encloses, and depends on the origin for an open one.
 *   Flipping a face swaps its columns 1 and 2; column 0 stays.
 *   vfn_orient_union_runs  reads keys[n_items] (sorted), nodes[n_items], dirs[n_items]; updates forest[n_nodes] (int32), which the
 *                     CALLER fills with x << 1: a word holds (parent << 1) | parity_to_parent, so that every load and every
 *                     compare-and-swap sees a consistent pair — hence n_nodes < 2^30.  One lane per item i >= 1: where
 *                     keys[i-1] == keys[i] >= 0, keys[i-2] and keys[i+1] (where they exist) differ from it and nodes[i-1] != nodes[i],
 *                     the trees of the two faces are united with the parity want = (dirs[i-1] != 0) == (dirs[i] != 0) between them — a
 *                     concurrent parity union-find (csrc/vfn_forest_core.h): only a root is ever hooked, by a compare-and-swap
 *                     (a, 0) -> (b, q) with b < a both found as roots; path halving by compare-and-swap composes the parities of the
 *                     skipped link.  A unite whose two finds end at one root writes nothing: conflicts are not judged here.  After the
 *                     launch the trees are the components, every root is its tree's lowest node, and in an orientable component the
 *                     parity of every node relative to its root is the unique one — whatever the schedule.  A node outside
 *                     [0, n_nodes): info bit 2, the pair is not followed.  A word whose parent lies outside [0, its node], or a root word
 *                     with its parity bit set (a forest that is not ours): info bit 2.
 *   vfn_orient_flatten  reads forest[n_nodes] AFTER the unions (another launch); writes root[n_nodes] (int64): where v's chain ends, and
 *                     parity[n_nodes] (uint8): the XOR of the parity bits along it.  Reads only.  A bad word: info bit 2, root[v] = -1,
 *                     parity[v] = 0.
 *   vfn_orient_votes  reads vertices[n, 3], faces[m, 3], parity[m] (NULL: all 0); one lane per face, its corners (v0, v1, v2) with
 *                     v1 and v2 exchanged where parity is set.
 *                     mode VFN_ORIENT_VOLUME (viewpoints NULL, n_views 0):
 *                       c = (v1.y v2.z - v1.z v2.y,  v1.z v2.x - v1.x v2.z,  v1.x v2.y - v1.y v2.x)      two products and one subtraction each
 *                       t = (v0.x c.x + v0.y c.y) + v0.z c.z
 *                     mode VFN_ORIENT_VIEWPOINTS (viewpoints[n_views, 3], n_views >= 1):
 *                       a = v1 - v0;  b = v2 - v0;  c = a x b as in vfn_face_normals;  g = ((v0 + v1) + v2) / 3      per coordinate
 *                       for j ascending: d = p_j - g;  s_j = (d.x d.x + d.y d.y) + d.z d.z;  the LOWEST j with the least s_j is taken
 *                       t = ((c.x d.x + c.y d.y) + c.z d.z) / sqrt(s);   t = 0 where s == 0
 *                     votes[m] = t.  One lane walks all the viewpoints — one per camera: a long list is slow and stays correct.  A
 *                     face with an index outside [0, n): info bit 2, votes = 0, nothing is read through it.  A non-finite coordinate
 *                     of the face or of a viewpoint: info bit 1.
 * info[0] (int64, zero-filled by the caller, only OR-ed into).  Limits: 1 <= n_nodes < 2^30, 1 <= n_items < 3 * 2^30, 0 <= n < 2^31,
 * 1 <= m < 2^31, 1 <= n_views < 2^31.  Every argument check answers before any launch.
 * ============================================================================================= */
#define VFN_ORIENT_VOLUME 0
#define VFN_ORIENT_VIEWPOINTS 1
int vfn_orient_union_runs(const int64_t* keys, const int64_t* nodes, const uint8_t* dirs, int64_t n_items, int32_t* forest, int64_t n_nodes,
                          int64_t* info, void* stream);
int vfn_orient_flatten(const int32_t* forest, int64_t n_nodes, int64_t* root, uint8_t* parity, int64_t* info, void* stream);
int vfn_orient_votes(const double* vertices, int64_t n, const int64_t* faces, int64_t m, const uint8_t* parity, int32_t mode,
                     const double* viewpoints, int64_t n_views, double* votes, int64_t* info, void* stream);

/* =============================================================================================
 * Vertex-clustering simplification of a triangle mesh (csrc/vfn_simplify.hip; vf_nerf_amd/meshops.py: simplify_vertex_clustering): the
 * vertices of every occupied voxel contracted into one, the faces that collapse dropped — what the reference does to a mesh before it
 * takes vertex_normals in get_dominant_bases (utils/utils.py:216-233).  A SPECIFICATION of ours that follows Open3D's
 * simplify_vertex_clustering (SimplificationContraction Average / Quadric) AS REMEMBERED: neither Open3D nor trimesh is available to
 * compare against, Open3D's hash map fixes no order of summation and its quadric solve has no in-cell test; ours do.  Everything is
 * float64, evaluated without contraction in the association written here, with no floating-point atomics: no bit depends on the
 * schedule.  Indices, keys and tables are int64.
 *   Clusters (the caller's, torch plumbing over the voxel unit above).  Only the vertices that some face names take part.  The frame is
 *                     the voxel unit's over THEIR bounding box: h = voxel_size, origin_k = min_k - 0.5 h.  A vertex's cell c and key are
 *                     vfn_voxel_keys'; clusters are numbered 0 .. K-1 in ascending key and the vertices of a cluster stand in ascending
 *                     index (the stable sort of the voxel unit).  The cell centre and the cluster mean:
 *                       g_k = origin_k + (c_k + 0.5) h                 an exact sum, a product, a sum; float64 elementwise
 *                       mean = vfn_voxel_means' mean of the cluster's vertices; colours and normals ride along as further channels
 *   vfn_face_planes   reads vertices[n, 3], faces[m, 3] and the HOST values origin[3]; one lane per face with corners (v0, v1, v2):
 *                       c = (v1 - v0) x (v2 - v0) as in vfn_face_normals;  s = c.x c.x;  s = s + c.y c.y;  s = s + c.z c.z;  r = sqrt(s)
 *                     r > 0 and finite:
 *                       nrm = (c.x / r, c.y / r, c.z / r)              three divisions
 *                       w = 0.5 r                                      the area
 *                       e = nrm.x (v0.x - origin.x);  e = e + nrm.y (v0.y - origin.y);  e = e + nrm.z (v0.z - origin.z)
 *                       planes[f, 0..4] = (nrm.x, nrm.y, nrm.z, e, w)
 *                     otherwise (a face without area, or a length that is not finite) planes[f, 0..4] = five +0.0.  info bits as
 *                     vfn_face_normals': bit 1 = a non-finite coordinate, bit 2 = a face index outside [0, n) (nothing is read through
 *                     it; five +0.0), bit 4 = r not finite.
 *   Items (the caller's).  The incidences (vertex, face), each once, ascending by vertex then face, sorted STABLY by the vertex's
 *                     cluster: a cluster's items stand in ascending (vertex, face).  item_face[n_items] names their faces and
 *                     start[K + 1] every cluster's first item and n_items.  For an item of cluster q with plane (nrm, e, w):
 *                       u_k = g_q,k - origin_k
 *                       d = nrm.x u.x;  d = d + nrm.y u.y;  d = d + nrm.z u.z;  d = d - e      the plane's signed distance from g_q
 *                       wn_i = w nrm_i;  wd = w d
 *                       its ten numbers:  wn_0 nrm_0, wn_0 nrm_1, wn_0 nrm_2, wn_1 nrm_1, wn_1 nrm_2, wn_2 nrm_2,      (A: a00 a01 a02 a11 a12 a22)
 *                                         wd nrm_0, wd nrm_1, wd nrm_2,                                             (b)
 *                                         wd d                                                                      (c)
 *                     so that the cluster's quadric about its cell centre is Q(x) = x^T A x + 2 b^T x + c, the area-weighted sum of the
 *                     squared distances of g_q + x from the planes of the cluster's faces.
 *   vfn_cluster_quadrics  reads planes[m, 5], item_face[n_items], start[K + 1], centres[K, 3] (= g), means[K, 3] and the HOST values
 *                     origin[3], h, rcond.  One WAVE of 64 lanes per cluster.  Each of the ten channels is added over the cluster's
 *                     items by vfn_cc_segment_sums' rule: lane t adds items b+t, b+t+64, ... serially from its FIRST one, a lane without
 *                     items holds +0.0, then s_t = s_t + s_(t+32) for t < 32, then 16, 8, 4, 2, 1.  Lane 0 then solves A x = -b by the
 *                     adjugate of the symmetric matrix:
 *                       m00 = a11 a22 - a12 a12;   m01 = a02 a12 - a01 a22;   m02 = a01 a12 - a02 a11
 *                       m11 = a00 a22 - a02 a02;   m12 = a01 a02 - a00 a12;   m22 = a00 a11 - a01 a01      two products, one subtraction
 *                       det = (a00 m00 + a01 m01) + a02 m02
 *                       y_0 = (m00 b0 + m01 b1) + m02 b2;  y_1 = (m01 b0 + m11 b1) + m12 b2;  y_2 = (m02 b0 + m12 b1) + m22 b2
 *                       x_k = -(y_k / det)
 *                       t = ((a00 + a11) + a22) / 3
 *                     The minimiser is ACCEPTED iff  det > rcond ((t t) t)  and  fabs(x_k) <= 0.5 h for k = 0, 1, 2; every comparison
 *                     is false on a NaN.  (The in-cell test is ours: a near-singular cluster can never throw its vertex out of its
 *                     cell.)  The output position and the offset z the error is taken at:
 *                       accepted:  position_k = g_k + x_k,  z = x;       otherwise:  position = mean (its bits),  z_k = mean_k - g_k
 *                       p_0 = (a00 z0 + a01 z1) + a02 z2;  p_1 = (a01 z0 + a11 z1) + a12 z2;  p_2 = (a02 z0 + a12 z1) + a22 z2
 *                       error = (((z0 p_0 + z1 p_1) + z2 p_2) + 2 ((b0 z0 + b1 z1) + b2 z2)) + c
 *                     placed[K] (uint8) is 1 where the minimiser was accepted.  The tables are not trusted: a segment that is empty,
 *                     decreasing or outside [0, n_items], or one that holds a face index outside [0, m), gets NaN in position and
 *                     error, placed 0 and info bit 2; nothing is read through such a bound or index.
 *   Faces (the caller's).  The input faces with every corner replaced by its cluster; faces that name a cluster twice are dropped, of
 *                     the faces with one sorted triple the lowest face index stays, the order and the winding of the others are
 *                     untouched; clusters that no remaining face names are dropped, the others keep their order.
 * info[0] (int64, zero-filled by the caller, only OR-ed into).  Limits: 0 <= n < 2^31, 1 <= m < 2^31, 1 <= n_items < 3 * 2^31,
 * 1 <= K <= n_items, h finite and > 0 with a normal square, rcond finite in [0, 1].  Every argument check answers before any launch.
 * ============================================================================================= */
int vfn_face_planes(const double* vertices, int64_t n, const int64_t* faces, int64_t m, const double* origin, double* planes, int64_t* info,
                    void* stream);
int vfn_cluster_quadrics(const double* planes, int64_t m, const int64_t* item_face, int64_t n_items, const int64_t* start, int64_t n_clusters,
                         const double* centres, const double* means, const double* origin, double voxel_size, double rcond,
                         double* position, uint8_t* placed, double* error, int64_t* info, void* stream);

/* =============================================================================================
 * Decimating a triangle mesh to a face count by quadric edge collapse (csrc/vfn_collapse.hip, csrc/vfn_collapse_core.h;
 * vf_nerf_amd/decimate.py: collapse_round, simplify_edge_collapse) — what the reference asks of trimesh's simplify_quadratic_decimation
 * in get_dominant_bases (utils/utils.py:227).  A SPECIFICATION of ours: a ROUND-BASED, MEMORYLESS quadric-error decimation, AS SPECIFIED
 * BY US, not verified against trimesh / Open3D and NOT their serial priority-queue order; the link condition is not tested (a known limit:
 * a collapse may make two faces name one vertex set, of which the later is dropped by the duplicate rule).  Everything is float64,
 * evaluated without contraction in the association written here, with no floating-point atomics: no output bit depends on the schedule.
 * Indices, keys and tables are int64.
 *   The call (the caller's, torch plumbing) first drops the faces that name a vertex twice and the later ones of a sorted triple, and
 *   fixes the frame's origin o as the lower corner of the bounding box of the vertices some face names.  It then repeats a ROUND, a pure
 *   function of (positions P[n, 3], faces F[m, 3] with m >= 1, the remaining budget):
 *   1 Planes.         Rows 0 .. m-1 are vfn_face_planes(P, F, o).  The 3m corner pairs — all (0,1), then all (1,2), then all (2,0) — with
 *                     key = min n + max are sorted stably; a run of equal keys is one undirected EDGE (a < b) = (key / n, key % n), edges
 *                     numbered 0 .. E-1 in ascending key, run[e] = the length of its run.  An edge with run 1 is a BOUNDARY edge: its one
 *                     pair names face f and the corners `from` then `to` in f's order.  The boundary edges, in ascending key, give the rows
 *                     m .. m+B-1 (vfn_boundary_planes, one lane each), with (nf, area) = planes[f, 0..2], planes[f, 4]:
 *                       d = P_to - P_from;   c = (d.y nf.z - d.z nf.y,  d.z nf.x - d.x nf.z,  d.x nf.y - d.y nf.x)
 *                       s = c.x c.x;  s = s + c.y c.y;  s = s + c.z c.z;  r = sqrt(s)
 *                     r > 0 and finite:  nrm = c / r (three divisions);  e = nrm.x (P_from.x - o.x);  e = e + nrm.y (..y);  e = e + nrm.z (..z);
 *                       row = (nrm.x, nrm.y, nrm.z, e, boundary_weight area)
 *                     otherwise five +0.0.  info bit 1 = a non-finite input, bit 2 = an index outside its range (nothing is read through
 *                     it; five +0.0), bit 4 = r not finite.
 *   2 Quadrics.       The ITEMS of a vertex are the rows it belongs to — the faces that name it, then the boundary rows of which it is an
 *                     end — in ascending row: item_row[n_items] with start[n + 1].  vfn_vertex_quadrics, ONE LANE per vertex: for a row
 *                     (nrm, e, w):  wn_i = w nrm_i;  we = w e;  its ten numbers
 *                       wn_0 nrm_0, wn_0 nrm_1, wn_0 nrm_2, wn_1 nrm_1, wn_1 nrm_2, wn_2 nrm_2,  -(we nrm_0), -(we nrm_1), -(we nrm_2),  we e
 *                     added channel by channel serially in item order STARTING from the first item (vfn_voxel_means' rule); a vertex
 *                     without items holds ten +0.0.  Q_v(z) = z^T A z + 2 b^T z + c is the weighted sum of the squared distances of o + z
 *                     from the vertex's planes.  A segment that is decreasing or outside [0, n_items], or a row outside [0, rows): ten
 *                     NaN and info bit 2.
 *   3 Candidates.     vfn_edge_collapse_candidates, one lane per edge (a, b) (csrc/vfn_collapse_core.h):
 *                       S = Q_a + Q_b channel by channel;  d = P_b - P_a;  l2 = (d.x d.x + d.y d.y) + d.z d.z;  mid_k = 0.5 (P_a,k + P_b,k)
 *                       m00 .. m22, det, y, x_k = -(y_k / det), t  exactly as in vfn_cluster_quadrics above
 *                       r_k = x_k - (mid_k - o_k);   r2 = (r.x r.x + r.y r.y) + r.z r.z
 *                     ACCEPTED iff  det > rcond ((t t) t)  and  r2 <= (reach reach) l2  (false on a NaN).  With value(z) = vfn_cluster_quadrics'
 *                     error at z over S:
 *                       accepted:   point_k = o_k + x_k,  value = value(x)
 *                       otherwise:  of (mid, P_a, P_b) in this order the one with the lowest value(point - o), replaced only by a
 *                                   strictly lower one; point = its bits
 *                       cost = value > 0 ? value : +0.0              so a cost's bit pattern orders like its value; -0.0 never appears
 *                       g = point - P_a;  s = ((g.x d.x + g.y d.y) + g.z d.z) / l2;  s = +0.0 unless s >= 0;  s = 1 where s > 1
 *                     flags[e] (uint8): 2 = accepted; 4 = run > 2 (a non-manifold edge); 8 = value or point not finite (and info bit 1);
 *                     16 = cost > max_error (max_error = +inf: no bound); and, only where none of 4, 8, 16 is set, the FLIP TEST: every
 *                     face in the items of a, then of b, that does not name the other end, with corners (p0, p1, p2):
 *                       c_old = (p1 - p0) x (p2 - p0) as in vfn_face_planes;  c_new = the same with the end replaced by point
 *                       the face passes iff  (c_old.x c_new.x + c_old.y c_new.y) + c_old.z c_new.z > 0;  c_old == (0, 0, 0) imposes nothing
 *                     32 = some face failed.  1 = the edge is a CANDIDATE: none of 4, 8, 16, 32.  An edge end, a segment, a row or a face
 *                     corner outside its range, or an item that does not name its vertex: info bit 2, no candidate, nothing is read
 *                     through it (ends outside [0, n) or a == b: point, cost and s are NaN).
 *   4 Selection.      vfn_collapse_select; its result is a function of the costs alone.  Every vertex CHOOSES among the candidates it is
 *                     an end of the lowest (cost, edge index): best_edge[n] (2^63 - 1: none; best_cost[n] is the workspace of the first
 *                     pass).  An edge is PROPOSED iff both its ends chose it.  Then every face takes the proposed edges its three
 *                     corners chose; if they are not all one edge, all but the lowest (cost, edge index) among them are WITHDRAWN.  Only
 *                     the proposals are used: the rule is not recursive.  What stays (proposed and not withdrawn) is a set of edges none
 *                     of whose 1-rings share a moving vertex, so the flip test of step 3 is exact when the collapse is applied; and the
 *                     globally lowest candidate always stays.
 *   5 Budget (the caller's).  The edges that stay, sorted ascending by (cost, edge index) (a stable sort of the costs over the index
 *                     order); with a target the shortest prefix whose summed run is >= m - target_faces is TAKEN, all of them if it
 *                     never gets there; without one, all.
 *   6 Apply (the caller's).  For a taken edge: b -> a, P[a] = point, attr[a] = (1 - s) attr[a] + s attr[b] (two products, one sum),
 *                     cost[a] = max(cost[a], cost[b], the edge's cost).  The faces are remapped, those that name a vertex twice and the
 *                     later ones of a sorted triple are dropped.
 *   7 Stop (the caller's).  m <= target_faces, a round without a taken edge, or max_rounds rounds.
 * info[0] (int64, zero-filled by the caller, only OR-ed into).  Limits: 1 <= n, m < 2^31, 1 <= count <= 3m, m <= rows <= 4m,
 * 1 <= E <= 3m, rcond in [0, 1], reach and boundary_weight finite and >= 0, max_error >= 0.  Every argument check answers before any
 * launch.
 * ============================================================================================= */
int vfn_boundary_planes(const double* vertices, int64_t n, const double* planes, int64_t m, const int64_t* face, const int64_t* from,
                        const int64_t* to, int64_t count, const double* origin, double boundary_weight, double* out, int64_t* info,
                        void* stream);
int vfn_vertex_quadrics(const double* planes, int64_t rows, const int64_t* item_row, int64_t n_items, const int64_t* start, int64_t n,
                        double* quadrics, int64_t* info, void* stream);
int vfn_edge_collapse_candidates(const double* vertices, int64_t n, const int64_t* faces, int64_t m, const double* quadrics,
                                 const int64_t* item_row, int64_t n_items, const int64_t* start, int64_t rows, const int64_t* edge_a,
                                 const int64_t* edge_b, const int64_t* run, int64_t n_edges, const double* origin, double rcond, double reach,
                                 double max_error, double* point, double* cost, double* s, uint8_t* flags, int64_t* info, void* stream);
int vfn_collapse_select(const double* cost, const uint8_t* flags, const int64_t* edge_a, const int64_t* edge_b, int64_t n_edges,
                        const int64_t* faces, int64_t m, int64_t n, int64_t* best_cost, int64_t* best_edge, uint8_t* proposed,
                        uint8_t* withdrawn, int64_t* info, void* stream);

/* =============================================================================================
 * Clustering points in space (csrc/vfn_kmeans.hip; vf_nerf_amd/cluster.py: kmeans; meshops.py: dominant_bases): Lloyd's k-means, the
 * step of get_dominant_bases (utils/utils.py:216-233) that the reference leaves to sklearn.cluster.KMeans after it has decimated a mesh
 * and taken its vertex_normals.  A SPECIFICATION of ours: the plain float64 Lloyd iteration from given seeds.  Held against
 * scikit-learn's KMeans(init = the same seeds, n_init = 1, algorithm = "lloyd", tol = 0) on the CPU: equal labels, equal iteration
 * counts, centres to rounding (tests/test_kmeans_host.py).  NOT verified: scikit-learn's own seeding (its greedy k-means++ and its
 * random stream) — the seeding below is ours.  Everything is float64, evaluated without contraction in the association written here,
 * with no floating-point atomics: every output bit is a function of the data alone.  points[n, 3] row-major, 1 <= n < 2^31,
 * 1 <= k <= VFN_KMEANS_MAX_K.  d2(p, c) = (dx dx + dy dy) + dz dz with dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z: the
 * association of vfn_nn_radius.
 *   vfn_kmeans_assign reads points, centres[k, 3] and previous[n] (int32, may be NULL); one lane per point.  label[i] (int32) = the j
 *                     with the least d2(p_i, c_j), a tie going to the LOWEST j (the comparison is strict, j ascending; all comparisons
 *                     are false on a NaN: label 0); sqdist[i] = that d2.  changed[0] (int64, device) is INCREASED by the number of
 *                     points with label[i] != previous[i] — every point when previous is NULL — by an integer atomic: the count does
 *                     not depend on the order.  previous and label may be the same array.  info bit 1 = a non-finite coordinate of a
 *                     point or a centre.
 *   vfn_kmeans_update reads points and label[n]; for every cluster j < k and c < 3:
 *                       sums[j, c] = THE FIXED TREE (above, after vfn_reduce_stats) over the n values label[i] == j ? p[i, c] : +0.0,
 *                                    lane order "near", P = ceil(n / 4096) partials per cluster
 *                       count[j]   = the number of i with label[i] == j (int64, exact)
 *                       centres[j, c] = sums[j, c] / (double)count[j]            where count[j] > 0
 *                     and a cluster with count 0 KEEPS its centre: centres[k, 3] is read and written, the bits of an empty cluster's row
 *                     are not touched; it shows in count.  A label outside [0, k): info bit 2, the point joins no cluster and nothing
 *                     is read through the label.  info bit 1 = a non-finite coordinate.
 *                     workspace: vfn_kmeans_update_workspace_bytes(n, k) bytes (the partials); -1 on error.
 *   vfn_kmeans_seed   one step of farthest-point or D^2 seeding without a host read.  newest[0] (int64, DEVICE memory) names the point q
 *                     that became a centre last:
 *                       mind2[i] = d2(p_i, p_q)                      first != 0
 *                       mind2[i] = min(mind2[i], d2(p_i, p_q))       first == 0   (old < d ? old : d)
 *                     then farthest[0] (int64, device) = the i with the greatest mind2[i], a tie going to the LOWEST i; -1 when no
 *                     mind2[i] compares (all NaN).  A maximum under a total order is associative and commutative: any reduction gives
 *                     these bits.  newest NULL: mind2 is read as it is and only the maximum is taken.  farthest NULL: only mind2 is
 *                     written (no workspace needed).  newest[0] outside [0, n): info bit 2, mind2 is left as it is, farthest[0] = -1
 *                     and nothing is read through the index.  info bit 1 = a non-finite coordinate.
 *                     workspace: vfn_kmeans_seed_workspace_bytes(n) bytes; -1 on error.
 * The inertia is vfn_reduce_stats' sum of sqdist.  info[0] (int64, zero-filled by the caller, only OR-ed into).  Every argument check
 * answers before any launch.
 * ============================================================================================= */
#define VFN_KMEANS_MAX_K 64           /* clusters of one call at most (a tile's presence mask is one 64-bit word) */
int vfn_kmeans_assign(const double* points, int64_t n, const double* centres, int32_t k, const int32_t* previous, int32_t* label,
                      double* sqdist, int64_t* changed, int64_t* info, void* stream);
int64_t vfn_kmeans_update_workspace_bytes(int64_t n, int32_t k);
int vfn_kmeans_update(const double* points, int64_t n, const int32_t* label, int32_t k, double* sums, int64_t* count, double* centres,
                      int64_t* info, void* workspace, int64_t workspace_bytes, void* stream);
int64_t vfn_kmeans_seed_workspace_bytes(int64_t n);
int vfn_kmeans_seed(const double* points, int64_t n, const int64_t* newest, int32_t first, double* mind2, int64_t* farthest,
                    int64_t* info, void* workspace, int64_t workspace_bytes, void* stream);

/* =============================================================================================
 * Optimizer side of a training step over ONE flat fp32 buffer (train/vector_field_nerf_train.py:254-260:
 * torch.nn.utils.clip_grad_norm_(model.parameters(), clip); optimizer.step()).  The unique parameters — and their gradients
 * and Adam moments — are laid out contiguously, sorted into up to four REGIONS [start, end) of equal multiplicity `mult` =
 * how often the parameter occurs in the optimizer's list (the reference lists every vector-field parameter twice,
 * models/nerf/vector_field_nerf.py:57-63): a gradient counts mult times in the norm, is scaled mult times, and its parameter
 * receives mult consecutive Adam updates per step, exactly what the sequential per-entry loops do.
 * vfn_flat_clip_grad_norm: out2[0] = total 2-norm, out2[1] = min(max_norm / (norm + 1e-6), 1), NaN where the norm is NaN
 *   (torch.clamp(max=1): every gradient inside the regions becomes NaN then; an infinite norm gives 0); gradients scaled in place.
 *   workspace: vfn_flat_clip_workspace_bytes() bytes of device memory, zero-filled once by the caller.
 * vfn_flat_adam_step: step_size[2 r + k] = lr / (1 - beta1^t), bc2_sqrt[2 r + k] = sqrt(1 - beta2^t) for update k (t = the step
 *   number of that update) of region r, evaluated by the caller in double precision as torch.optim.Adam does. */
int64_t vfn_flat_clip_workspace_bytes(void);
int vfn_flat_clip_grad_norm(float* flat_grad, int64_t n, int32_t n_regions, const int64_t* starts, const int64_t* ends,
                            const int32_t* mults, float max_norm, void* workspace, float* out2, void* stream);
int vfn_flat_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t n_regions,
                       const int64_t* starts, const int64_t* ends, const int32_t* mults, const double* step_size,
                       const double* bc2_sqrt, double beta1, double beta2, double eps, double weight_decay, void* stream);

/* =============================================================================================
 * ONE training step in ONE call (csrc/vfn_train.hip): the reference trainer's loop body, train/vector_field_nerf_train.py:172-260 in the
 * regime every shipped scene runs (eval-mode networks, :140-141; border + centre supervision, :186-216; VFLoss; zero_grad; backward;
 * clip_grad_norm_ over the duplicated parameter list; Adam.step) issued from C on one stream out of one caller-supplied workspace —
 * what vfn_render_fwd is to the gradient-free render().  It SEQUENCES entry points of this header (the f16x3 saving forwards with one
 * vector-field evaluation per distinct sample, vfn_vf_loss_fwd / _bwd, the bf16 chains over one fragment-ordered workspace shared by
 * the fine pass and the supervision batch, vfn_net_weight_grads_frag_part, vfn_flat_clip_grad_norm, vfn_flat_adam_step, the re-packs),
 * so every value is what those entry points produce called one by one.
 *   phases: VFN_TRAIN_FORWARD_BACKWARD ends with every parameter's gradient ADDED into flat_grad (zeroed first); a multi-rank caller
 *           all-reduces flat_grad, then calls again with VFN_TRAIN_OPTIMIZER (clip, Adam, re-pack).  Both bits: the whole step.
 *   render: sizes, samplers, density, Philox (seed, offset) of the three draws (laid out coarse | fine | add, as vfn_render_fwd);
 *           colour_products / separate_launches / timing_events are ignored; streams >= 2: the supervision batch's forward and chain
 *           run on an internal side stream forked from / joined into `stream` (same values).  N S_c and N S_t must be multiples of 32.
 *   loss:   weights, clamp and flags of VFLoss; n_rays / n_normals / n_sup are filled in by the call (ONE supervision segment: the
 *           border batch followed by the centre batch; ray_center selects the ray samples inside the centre ball on the device).
 *   n_sup:  points per supervision batch (the trainer uses (N S_t) / 10); border / center: which batches exist; the shells are
 *           [border_r_min, border_r_max] (inward ground truth) and [0, sup_radius] (outward) around sup_centroid; their draws come
 *           from the Philox stream (sup_seed, sup_offset) — border first — unless sup_u_border / sup_u_center supply them ([n_sup,3]).
 *   save_flags / dy_flags / dy_form / x_form: the storage forms of the training workspace (vfn_vf_render_fused16_fwd_train_at,
 *           vfn_mlp_bwd_chain_bf16_ws_at, vfn_weight_grad_frag); fragment order (save_flags bit 1) is required.
 *   forward_products: colour_products of the saving forwards (3; 2; 1 = the single-product mode, which also takes dy_flags bit 4).
 *   regions / step_size / bc2_sqrt / betas / eps / weight_decay / max_norm: as vfn_flat_clip_grad_norm and vfn_flat_adam_step.
 *   repack: re-pack vf_packed16, rn_packed16 and the two transposed bf16 packs from the updated parameters at the end of phase 2.
 *   sparse_colours: a sample's colour enters the step through rgb = sum_s w_s c_s only, so where w_s is exactly zero — a closed density
 *           ReLU, or a transmittance that has underflowed: 93-97 % of the samples of a batch — neither the colour nor its gradient
 *           (d c_s = w_s d rgb) nor the rendering net's share of that sample in any weight gradient is needed, and every derivative of w_s
 *           that would multiply c_s ends at the closed ReLU / the zero transmittance.  With sparse_colours the step evaluates the
 *           vector-field net on all samples with its vector-only saving forward (region 1 of the workspace), selects on the device the
 *           samples whose colour can reach an output or a gradient — w > 0, or w = 0 by an underflowed alpha alone (sigma > 0, delta > 0
 *           and a non-zero transmittance: alpha = 1 - exp(-sigma delta) rounds to 0 for sigma delta < 3e-8 while d w / d sigma = T delta
 *           does not, and the dense step's (d rgb . c_s) T delta term of that sample's d sigma needs c_s) — a count the host never learns
 *           (launches are sized for the capacity and cut inside the kernels), and runs the fused saving forward, the fused chain and the
 *           colour branch's weight gradients on that compacted list only (region 2).
 *           The upstream gradient splits between the regions (d normals on region 1, d colours on region 2): the parameter gradients are
 *           the dense step's up to the order of their sums; rgb, depth, weights, normals are the dense step's bit for bit; the `colors`
 *           output holds zeros on the samples that were not selected (vf_nerf_amd fills them on first access of NerfOutput.coarse_colors).
 * Outputs of phase 1 (caller-allocated, the NerfOutput of the step's render): ray_dirs[N,3], z_vals[N,S_t], points[N,S_t,3],
 * normals[N S_t,3], colors[N S_t,3], weights[N,S_t], rgb[N,3], depth[N]; out_terms[8] as vfn_vf_loss_fwd; out_counts[2] (optional) =
 * the number of samples the colour branch was evaluated for (sparse_colours: the selected ones) and N S_t.  Phase 2: out_norm[2] as
 * vfn_flat_clip_grad_norm.  No allocation, no synchronisation, no host read-back.
 *
 * SESSION FORM (ABI 4): the same step for a caller that makes the reference trainer's calls ONE BY ONE — render(), the two supervision
 * forwards, the loss, backward(), clip, step (train/vector_field_nerf_train.py:177-260 unchanged, through vf_nerf_amd.dropin) — and still wants
 * the step's launches: same workspace, same kernels, the caller's own loss in the middle.
 *   VFN_TRAIN_RENDER    the render() part of phase 1 alone (prep, rays, saving forwards, selection, composite).  sup_rows_reserved (a
 *                       multiple of 32) rows of the workspace are set aside for supervision batches appended later; their points and
 *                       upstream-gradient rows are zeroed.
 *   vfn_train_step_supervision_points / _forward: one supervision batch into rows [row0, row0 + count) of that region (sampled by the call as
 *                       phase 1 samples them) and its vector-only saving forward over rows [row0, pad32(row0 + count)) (row0 a multiple of 32).
 *                       With render.streams >= 2 they run on the calling thread's side stream, ordered after this step's prep launch, beside
 *                       the render's launches, and are joined into `stream` before the call returns.  The caller reads predictions / ground
 *                       truth / points at the offsets vfn_train_step_workspace_layout reports and leaves the loss's gradient with respect to the
 *                       predictions in the D_SUP rows.
 *   VFN_TRAIN_BACKWARD  the backward part of phase 1 alone, from upstream gradients the caller supplies: io->d_rgb_in[N,3], io->d_depth_in[N]
 *                       (or NULL), io->d_normals_in[N S_t,3] over the SORTED samples (copied into the workspace's DN rows unless it already is
 *                       that address) and the D_SUP rows.  Gradients are ADDED into flat_grad / g_beta / g_mean / g_scale (the caller's
 *                       zero_grad() decides what they start from).
 * vfn_train_step_workspace_layout: out[VFN_TWS_*] for the given sizes — byte offsets into the workspace, or counts. */
#define VFN_TRAIN_FORWARD_BACKWARD 1
#define VFN_TRAIN_OPTIMIZER 2
#define VFN_TRAIN_RENDER 4
#define VFN_TRAIN_BACKWARD 8
#define VFN_TRAIN_CLIP 16         /* the two halves of VFN_TRAIN_OPTIMIZER: clip_grad_norm_ (out_norm) ...                 */
#define VFN_TRAIN_ADAM 32         /* ... and optimizer.step (+ the re-pack), for a caller that makes them as two calls */
#define VFN_TWS_SUP_PTS 0        /* float[rows][3]  supervision points                                            */
#define VFN_TWS_SUP_GT 1         /* float[rows][3]  their radial ground truth                                     */
#define VFN_TWS_SUP_PRED 2       /* float[rows][3]  vector head of the supervision rows                           */
#define VFN_TWS_D_SUP 3          /* float[rows][3]  upstream gradient of those predictions                        */
#define VFN_TWS_DN 4             /* float[N S_t][3] upstream gradient of the sorted normals                       */
#define VFN_TWS_SUP_ROWS 5       /* count: rows of the supervision region                                         */
#define VFN_TWS_TOTAL_ROWS 6     /* count: points of one fragment-ordered slot                                    */
#define VFN_TWS_BYTES 7          /* = vfn_train_step_workspace_bytes                                              */
#define VFN_TWS_COUNT 8
typedef struct vfn_train_step_params {
    vfn_render_params render;
    vfn_loss_params loss;
    int64_t n_sup;
    int32_t border, center;
    float sup_centroid[3];
    float sup_radius;                   /* centre ball [0, sup_radius] (outward ground truth); also the radius of the ray_center selection */
    float border_r_min, border_r_max;   /* border shell (inward ground truth): far - 5 radius .. far, evaluated by the host in double as Python does */
    int32_t phases;
    uint64_t sup_seed, sup_offset;
    int32_t save_flags, dy_flags, dy_form, x_form;
    int32_t forward_products;
    int32_t repack;
    int32_t n_regions;
    int32_t mults[4];
    int64_t starts[4], ends[4];
    double step_size[8], bc2_sqrt[8];
    double beta1, beta2, eps, weight_decay;
    float max_norm;
    int32_t sparse_colours;             /* != 0: the colour branch (feature block + rendering net) is evaluated, differentiated and summed into the
                                         * weight gradients only for the samples whose weight is non-zero (see below) */
    int64_t sup_rows_reserved;          /* session form: rows (a multiple of 32) of the supervision region; 0: pad32(n_sup (border + center)) */
    int64_t sup_rows_used;              /* session form, VFN_TRAIN_BACKWARD: the leading rows (a multiple of 32, <= sup_rows_reserved) of that region that
                                         * supervision forwards have filled — the chain and the weight gradients walk these and no others (a row no
                                         * forward has written holds no activations) */
} vfn_train_step_params;
typedef struct vfn_train_step_io {
    const vfn_net_geom* vf_geom; const vfn_net_geom* rn_geom;
    void* vf_packed16; void* rn_packed16; void* vf_packed_bwd16; void* rn_packed_bwd16;       /* read by phase 1, rewritten by the re-pack */
    const vfn_layer_params* vf_layers; const vfn_layer_params* rn_layers;                     /* host arrays [n_layers]: the re-pack's inputs */
    const vfn_wgrad_layer* vf_wgrad; const vfn_wgrad_layer* rn_wgrad;                         /* host arrays [n_layers]: parameters and where their gradients go */
    const float* vf_head_w; const float* rn_head_w;                                           /* rows 0..2 of each net's last Linear */
    const float* beta; const float* mean; const float* scale;                                 /* the density's three raw scalars ... */
    float* g_beta; float* g_mean; float* g_scale;                                             /* ... and their gradient words (inside flat_grad) */
    float* flat_param; float* flat_grad; float* exp_avg; float* exp_avg_sq; int64_t n_flat;   /* the optimizer's flat buffers (vfn_flat_adam_step) */
    void* clip_workspace;
    const float* uv; const float* pose; const float* intrinsics; const float* t_vals;
    const float* far_coarse_per_ray; const float* far_fine_per_ray;
    const float* u_coarse; const float* u_fine; const float* u_add;                           /* optional supplied draws (parity runs) */
    const float* sup_u_border; const float* sup_u_center;
    const float* rgb_gt; const float* depth_gt;
    void* workspace;                                                                          /* vfn_train_step_workspace_bytes() bytes */
    float* ray_dirs; float* z_vals; float* points; float* normals; float* colors; float* weights; float* rgb; float* depth;
    float* out_terms; float* out_norm;
    float* out_counts;                                                                        /* optional [2]: samples the colour branch ran on, all samples */
    const float* d_rgb_in; const float* d_depth_in; const float* d_normals_in;                /* VFN_TRAIN_BACKWARD: the caller's upstream gradients */
} vfn_train_step_io;
int64_t vfn_train_step_workspace_bytes(const vfn_train_step_params* p, const vfn_net_geom* vf_geom, const vfn_net_geom* rn_geom);
int vfn_train_step(const vfn_train_step_params* p, const vfn_train_step_io* io, void* stream);
int vfn_train_step_workspace_layout(const vfn_train_step_params* p, const vfn_net_geom* vf_geom, const vfn_net_geom* rn_geom, int64_t* out, int32_t n_out);
/* vfn_sample_sphere_shell into rows [row0, row0 + count) of the open step's supervision region (points and ground truth).  The centre is
 * given BY VALUE (cx, cy, cz) — then, with Philox draws (u == NULL), the launch depends on nothing the caller's stream produced after the
 * step's prep and runs on the side stream — or as a device pointer centroid_dev / with supplied draws u[count,3], and then on `stream`.
 * Returns 1 (not an error) when it ran on the side stream, 0 when on `stream`: pass that as on_side to the forward of the same rows.
 * vfn_train_step_supervision_forward: the vector-only saving forward over rows [row0, pad32(row0 + count)), predictions into the SUP_PRED rows. */
int vfn_train_step_supervision_points(const vfn_train_step_params* p, const vfn_train_step_io* io, int32_t inward, float r_min, float r_max,
                                      float cx, float cy, float cz, const float* centroid_dev, int64_t row0, int64_t count, const float* u,
                                      uint64_t seed, uint64_t offset, void* stream);
int vfn_train_step_supervision_forward(const vfn_train_step_params* p, const vfn_train_step_io* io, int64_t row0, int64_t count, int32_t on_side,
                                       void* stream);
/* The backward of supervision rows [row0, pad32(row0 + count)) ALONE (their upstream gradient in the D_SUP rows): the vector-only chain and the
 * vector-field net's weight gradients of those rows, added into flat_grad; the D_SUP rows are zeroed afterwards.  For a backward pass that
 * never reaches VFN_TRAIN_BACKWARD (a loss that uses the supervision predictions only). */
int vfn_train_step_supervision_backward(const vfn_train_step_params* p, const vfn_train_step_io* io, int64_t row0, int64_t count, void* stream);

/* =============================================================================================
 * Networks in TRAINING mode: nn.BatchNorm1d with batch statistics (vector_field_network.py:146-208 and
 * rendering_network.py:62-108 after VectorFieldNerf.train(), vector_field_nerf.py:139-150; the trainer enters it when the
 * directional-derivative loss weight is non-zero, train/vector_field_nerf_train.py:140-141).  Batch statistics couple all
 * rows of a layer, so the layers run one launch at a time on row-major fp32 matrices in HBM.  Leading dimensions are
 * multiples of 4 floats, rows 16-byte aligned, pad columns hold zeros.
 * ============================================================================================= */
/* (transpose_w is a bit field: bit 0 = the transposition below; bits 1-2 = the arithmetic — 0: exact fp32 (v_mfma_f32_32x32x2f32); 2: SPLIT
 *  f16, every operand as two f16 halves and a product as a_hi b_hi + a_hi b_lo + a_lo b_hi on v_mfma_f32_32x32x16_f16 with fp32
 *  accumulation, 22 significant bits, for forward GEMMs on normalised activations (A rides at 64x its value so that its low halves stay
 *  out of the f16 denormals: |A| must stay below 1023, |W| below 65504 — batch-normalised activations, encodings, points and weights
 *  do; gradients do not, hence form 6 for the backward products); 4: SPLIT bf16, the same with bf16 halves, 16 significant
 *  bits and fp32's exponent range; 6: bf16 in THREE parts (hi | mid | lo = 24 bits), six products: fp32-equivalent at fp32's exponent
 *  range, for backward GEMMs on gradients of any magnitude.  5.3x / 5.3x / 2.7x fewer matrix cycles than the exact form; A goes through LDS
 *  in whole cache lines in these forms.)
 * transpose_w = 0: C[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]), W = nn.Linear weight [n_out][ldw], k_in columns
 *                  (torch.nn.functional.linear); act 0 none / 1 tanh / 2 sigmoid.
 * transpose_w = 1: C[m][j] = sum_k A[m][k] W[k][j], W [k_in][ldw], j < n_out  (the input gradient dX = dZ W).
 * A is read over k rounded up to a multiple of 8 (lda must cover it, pad columns zero).
 * stats_part (or NULL): [vfn_linear_rows_stat_parts(m)][2][n_out] per-workgroup column sums of the pre-activation z and
 * of z^2 — the batch statistics, finished by vfn_colsum_finish. */
int vfn_linear_rows(int32_t transpose_w, const float* a, int32_t lda, const float* w, int32_t ldw, const float* bias,
                    int64_t m, int32_t n_out, int32_t k_in, int32_t act, float* c, int32_t ldc, float* stats_part,
                    void* stream);
/* vfn_linear_rows with a scratch for W's 16-bit planes (vfn_linear_rows_wplanes_bytes(n_out, k_in) bytes, 16-byte aligned; NULL: as
 * vfn_linear_rows).  The split arithmetics with two planes (transpose_w & 6 = 2, 4) then split W ONCE per call — one small launch in front of
 * the product — instead of once per workgroup and chunk; same values bit for bit.  The scratch is free again when the call's launches have run. */
int vfn_linear_rows_ws(int32_t transpose_w, const float* a, int32_t lda, const float* w, int32_t ldw, const float* bias,
                       int64_t m, int32_t n_out, int32_t k_in, int32_t act, float* c, int32_t ldc, float* stats_part,
                       void* wplanes, void* stream);
int64_t vfn_linear_rows_wplanes_bytes(int32_t n_out, int32_t k_in);
int64_t vfn_linear_rows_stat_parts(int64_t m);
/* A forward layer product with the PREVIOUS layer's BatchNorm + ReLU folded into its operand read (round 6, ABI 5):
 * C[M, n_out] = act(z_prev) W^T + bias with act(z)[k] = post_prev * max(z[k] * scale[k] + shift[k], 0) for k < n_prev (coef_prev =
 * [4][n_prev]) and post_prev * z[k] for n_prev <= k < k_in; arith 2 (three f16 products on split operands); 129 <= n_out <= 256;
 * stats_part as vfn_linear_rows_ws; wplanes (its scratch for W's planes) is required.  Replaces the vfn_bstat_relu_rows pass + vfn_linear_rows_ws pair of a training-mode layer
 * (models/vector_field/vector_field_network.py:177-208 with batch statistics): same operand values, one [M, 256] write and read less. */
int vfn_linear_rows_fold(int32_t arith, const float* z_prev, int32_t ldz, const float* coef_prev, int32_t n_prev, float post_prev,
                         const float* w, int32_t ldw, const float* bias, int64_t m, int32_t n_out, int32_t k_in, float* c, int32_t ldc,
                         float* stats_part, void* wplanes, void* stream);
/* The input-gradient product C[m][n_out] = dZ[m][k_in] W[k_in][n_out] (vfn_linear_rows with transpose_w = 1 | arith; arith = 4: three
 * bf16 products, 16 significant bits at fp32's exponent range — the arithmetic of the eval-mode dX chain, the default since round 5 — or
 * 6: bf16 in three parts, six products, 24 bits) that
 * also leaves, while C is in registers, the per-workgroup partials sums_part[vfn_linear_rows_stat_parts(m)][2][n_prev] of sum g' and
 * sum g' x_hat of the PREVIOUS layer's BatchNorm backward over the first n_prev (<= 256) columns of C — g' = post_prev C [z_prev scale +
 * shift > 0], x_hat = (z_prev - mean) rstd with coef_prev [4][n_prev] = scale, shift, mean, rstd — i.e. what vfn_bstat_relu_bwd_sums
 * computes in a pass of its own; finished by vfn_colsum_finish(sums_part, parts, 2 n_prev).  wplanes: as vfn_linear_rows_ws (or NULL).
 * Reference: the autograd of nn.Linear + nn.BatchNorm1d (training) + ReLU, models/vector_field/vector_field_network.py:176-208. */
int vfn_linear_rows_dx_sums(const float* dz, int32_t lddz, const float* w, int32_t ldw, int64_t m, int32_t n_out, int32_t k_in, float* c,
                            int32_t ldc, const float* z_prev, int32_t ldz_prev, const float* coef_prev, int32_t n_prev, float post_prev,
                            float* sums_part, int32_t arith, void* wplanes, void* stream);
/* Partials per workgroup of the row-wise kernels below (vfn_bstat_relu_bwd_sums). */
int64_t vfn_bstat_row_parts(int64_t m);
/* part[n_parts][width] fp32 -> sums[width] double. */
int vfn_colsum_finish(const float* part, int64_t n_parts, int32_t width, double* sums, void* stream);
/* sums[2][n] (sum z, sum z^2 over m rows) -> coef[4][n] = scale (gamma rstd), shift (beta - mean scale), mean, rstd with
 * rstd = 1 / sqrt(biased variance + eps); running_mean / running_var (may be NULL) <- (1 - momentum) old + momentum batch,
 * the variance unbiased (m / (m - 1)), as torch.nn.BatchNorm1d does in training mode. */
int vfn_bstat_finalize(const double* sums, int64_t m, int32_t n, const float* gamma, const float* beta, float eps,
                       float momentum, float* running_mean, float* running_var, float* coef, void* stream);
/* h[m][c] = post_scale * relu(z[m][c] * scale[c] + shift[c]), c < n. */
int vfn_bstat_relu_rows(const float* z, int32_t ldz, const float* coef, int64_t m, int32_t n, float post_scale, float* h,
                        int32_t ldh, void* stream);
/* Backward of the above through the batch statistics.  g = gradient wrt h.  With g' = post_scale g [z scale + shift > 0] and
 * x_hat = (z - mean) rstd:  part[vfn_bstat_row_parts(m)][2][n] = per-workgroup sums of g' and g' x_hat (= d beta, d gamma
 * after vfn_colsum_finish);  dz = gamma rstd (g' - sum g' / m - x_hat sum(g' x_hat) / m). */
int vfn_bstat_relu_bwd_sums(const float* g, int32_t ldg, const float* z, int32_t ldz, const float* coef, int64_t m, int32_t n,
                            float post_scale, float* part, void* stream);
int vfn_bstat_relu_bwd_rows(const float* g, int32_t ldg, const float* z, int32_t ldz, const float* coef, const double* sums,
                            int64_t m, int32_t n, float post_scale, float* dz, int32_t lddz, void* stream);
/* dz = dy (1 - y^2) (act 1, tanh) or dy y (1 - y) (act 2, sigmoid) or dy (act 0).  dy == NULL: dy is 1 in column
 * onehot_col and 0 elsewhere — the grad_outputs of the three autograd.grad calls of vector_field_network.py:150-171. */
int vfn_act_bwd_rows(int32_t act, const float* dy, int32_t lddy, const float* y, int32_t ldy, int64_t m, int32_t n,
                     int32_t onehot_col, float* dz, int32_t lddz, void* stream);
/* dst[row][col0 + j] = scale * PE(src3[row / rows_per_src])[j], j < 3 + 6 multires (models/helpers/embedder.py:11-37;
 * multires 0 copies the 3 values). */
int vfn_embed_rows(const float* src3, int32_t ld_src, int32_t rows_per_src, int64_t m, int32_t multires, float scale,
                   float* dst, int32_t ld_dst, int32_t col0, void* stream);
/* d_src3[m][3] (+)= sum over the (up to two) places the encoding was used of scale * dPE/dx applied to the gradient
 * rows d[row][col..col+3+6 multires) (d_b may be NULL). */
int vfn_embed_rows_bwd(const float* src3, int64_t m, int32_t multires, const float* d_a, int32_t ld_a, int32_t col_a,
                       float scale_a, const float* d_b, int32_t ld_b, int32_t col_b, float scale_b, float* d_src3,
                       int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VFN_H */
