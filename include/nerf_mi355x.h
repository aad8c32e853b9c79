/*
 * nerf_mi355x.h - C ABI of the MI355X-native NeRF ray-chunk renderer.
 *
 * The reference (isaacchunn/nerf-projects, nerf/) has no FFI or plugin layer on this
 * path: its "operator API" is the set of Python signatures in notebook cells 8-12/15 of
 * nerf/nerf.ipynb plus nerf/nerf.py, nerf/embedder.py and nerf/nerf_helpers.py
 * (SURVEY.md section 8b). Each entry point below states the reference callable it
 * replaces; nerf-projects_amd/host.py binds them with ctypes under the reference's own
 * names and signatures, and INTEGRATION.md shows the stub a maintainer would add.
 *
 * Conventions
 *   - Every function returns 0 on success, a negative NERF_E_* code on failure, or a positive
 *     NERF_W_* warning (work done, outputs valid); nerf_last_error() returns a thread-local
 *     message for the last failure or warning.
 *   - Pointers marked [dev] are device (HBM) addresses on the context's GPU; [host]
 *     are ordinary host addresses. All arrays are dense row-major fp32.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream). Calls
 *     enqueue work and return; they do not synchronise. Outputs are complete when the
 *     stream reaches the point after the call (the reference is synchronous only
 *     because eager PyTorch on one stream is).
 *   - One context per GPU. A context owns the packed weights and ONE scratch workspace (grown on
 *     demand) that nerf_render_rays / nerf_render_frame / nerf_render_shard / nerf_train_step /
 *     nerf_image_metrics all reuse. Those calls may come from several streams or host threads:
 *     the library orders them itself (a mutex around the enqueue; a call on another stream than
 *     the previous one first waits, on the device, for an event recorded after the previous
 *     call), so they never overlap on the scratch - and therefore never overlap each other; for
 *     concurrent renders on one GPU create one context per stream. Weight loading
 *     (nerf_load_weights, nerf_set_adam_state) is not ordered against rendering on other
 *     streams: finish it (or synchronise) first.
 *   - No CPU fallback exists: without a gfx950 device nerf_ctx_create fails.
 */
#ifndef NERF_MI355X_H
#define NERF_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERF_OK 0
#define NERF_E_INVALID (-1)     /* bad argument / unsupported configuration */
#define NERF_E_HIP (-2)         /* a HIP runtime call failed                */
#define NERF_E_STATE (-3)       /* e.g. weights of a slot not loaded        */
#define NERF_E_NOMEM (-4)
/* Positive codes are warnings: the call did its work and the outputs are valid (see "Precision guard" below). */
#define NERF_W_PRECISION 1            /* the fp16-pair kernel's scale bound was loose in this call; outputs are its own   */
#define NERF_W_PRECISION_FALLBACK 2   /* ... and the work was redone (frame) / is being done from now on (training) in fp32 */

#define NERF_MAX_SKIPS 8
#define NERF_SLOT_COARSE 0      /* network_fn   (nerf.ipynb:887-889) */
#define NERF_SLOT_FINE 1        /* network_fine (nerf.ipynb:892-896) */
#define NERF_NUM_SLOTS 16

typedef struct nerf_ctx nerf_ctx;

/* Constructor arguments of the reference NeRF module (nerf/nerf.py:9). */
typedef struct nerf_arch {
    int32_t D;                  /* trunk depth, netdepth                          */
    int32_t W;                  /* trunk width, netwidth: 2..256. Inference runs a narrower network zero-padded to 256
                                   (the same function, at the 256-wide cost); a narrower network trains too, layer by
                                   layer and not on the fused fp16-pair kernels */
    int32_t input_ch;           /* 3 + 6*multires (63), or 3 for i_embed == -1    */
    int32_t input_ch_views;     /* 3 + 6*multires_views (27), or 3                */
    int32_t output_ch;          /* 4, or 5 when N_importance > 0 (nerf.ipynb:885) */
    int32_t n_skips;
    int32_t skips[NERF_MAX_SKIPS];
    int32_t use_viewdirs;
} nerf_arch;

/* Library / device ------------------------------------------------------------------ */

const char* nerf_last_error(void);
const char* nerf_version(void);
/* Number of visible HIP devices, or a negative error. */
int nerf_device_count(void);

/* Create a context on HIP device `device` (must be gfx950). */
int nerf_ctx_create(int device, nerf_ctx** out);
void nerf_ctx_destroy(nerf_ctx* ctx);

/* Arithmetic of the fused encode+MLP kernel (NeRF.forward, nerf/nerf.py:57-111). Inputs, outputs, biases,
 * activations between layers and everything outside the MLP are fp32 in both modes (the reference sets
 * torch.float32, nerf.ipynb:76); the modes differ in how the 256-wide contractions are evaluated:
 *   NERF_PRECISION_F32    v_mfma_f32_32x32x2_f32: an fp32 fmaf chain (24-bit operands).
 *   NERF_PRECISION_F16X2  every operand v carried as two fp16 numbers, hi = rn16(v), lo = rn16(v - hi), scaled per
 *                         layer (weights) and per point (activations) by powers of two so that nothing leaves the
 *                         fp16 range; three v_mfma_f32_32x32x16_f16 products per term (W_lo x_hi + W_hi x_lo +
 *                         W_hi x_hi, each exact in the fp32 accumulator), fp32 accumulation. What is proven:
 *                         |v - hi - lo| <= 2^-23 |v| (the remainder v - hi has up to 12 significant bits, lo keeps
 *                         11: up to one fp32 ulp is lost, none when the remainder fits) and the dropped W_lo x_lo is
 *                         <= 2^-22 |W x| per product. That is a per-product bound about 4x the fp32 rounding unit;
 *                         what is MEASURED is that through the whole network the error against an fp64 evaluation
 *                         is equal or smaller than the fp32 MFMA chain's (rms <= 1.25x, max <= 2x, asserted by
 *                         tests/test_hip_parity.py::test_mlp_precisions_vs_fp64 incl. adversarial scalings), because
 *                         these errors are unbiased and far below the accumulated rounding of a 256-term fp32 sum.
 *                         Scale groups: a weight more than 2^12 below the largest of its LAYER, or an activation
 *                         more than 2^12 below the largest of its POINT, has a low half in the fp16 subnormal
 *                         range (absolute resolution 2^-24 of the scaled unit) and keeps fewer than 24 bits. So
 *                         that hidden units of very different size do not meet in one group, the kernel evaluates
 *                         a ROW-EQUALISED copy of the network, made at load time and after optimiser steps: unit j
 *                         is scaled by 2^e_j to the median row norm (weights and bias) of its layer and column j of every layer that
 *                         reads it by 2^-e_j - the same function exactly (ReLU commutes with positive factors, the
 *                         factors are powers of two); nerf_get_weights returns the plain parameters. With it one
 *                         row of a layer 2^20 larger than the others costs nothing, whether its output is used or
 *                         not (tests/test_hip_parity.py::test_fp16_pair_rows_of_unequal_size). What remains is
 *                         WITHIN a row (a weight 2^12 below the layer's largest matters only when the inputs of
 *                         the large ones vanish) and within a point (units equal in norm but 2^12 apart on that
 *                         point); nerf_precision_status counts the points whose scale bound was that loose.
 * A context starts in NERF_PRECISION_F16X2 (about 3x the frame rate of the fp32 chain).
 * Takes effect for the following calls on this context; weights loaded earlier stay valid. */
#define NERF_PRECISION_F32 0
#define NERF_PRECISION_F16X2 1
int nerf_set_precision(nerf_ctx* ctx, int precision);
int nerf_get_precision(nerf_ctx* ctx);
/* The same for the RENDERING entry points only (nerf_render_rays / _frame / _shard and the stage calls): the training
 * step keeps the arithmetic nerf_set_precision chose and any fp32 fallback it is in. This is what a caller that re-renders a
 * range in fp32 after a precision warning uses (the Python mirror's batchify_rays): a validation render inside a training
 * loop must not put the loop back on the fp16-pair kernels. nerf_get_precision returns the rendering arithmetic. */
int nerf_set_render_precision(nerf_ctx* ctx, int precision);
/* View fold (NERF_PRECISION_F16X2, inference launches of view-dependent networks). feature_linear (nerf/nerf.py:89) has no
 * activation and views_linears.0 is its only consumer, so the forward kernel evaluates the view layer straight on the trunk
 * output: pre = W_vf h + W_v[:, W:] gamma(d) + b_vf with W_vf = W_v[:, :W] W_f, b_vf = W_v[:, :W] b_f + b_v, formed on the
 * device in fp64 and rounded once whenever the fp16-pair data are rebuilt (at load, after optimiser steps) - 66 weight
 * chunks per 32 points instead of 74; sigma (alpha_linear on the trunk output) is computed as before, bit for bit. A
 * network is folded only when every parameter involved and the fold are finite, feature_linear cannot overflow for trunk
 * outputs up to 2^64, and the two column blocks of the folded layer are within 2^8 of each other in size; otherwise it runs
 * the three layers one after the other, as do the fp32 kernel and the training passes always (they keep the feature vector
 * for the backward pass). nerf_render_rays with random draws (perturb, noise0 / noise) does not fold either: it is the
 * render nerf_train_forward and nerf_train_step reproduce bit for bit. A taped render without random draws differs from
 * the untaped one in the colours by the fold's rounding (within 2e-5 in rgb_map). The one deviation: where the
 * reference's feature vector would overflow fp32 on a trunk output beyond that range, the folded kernel counts a
 * loose-bound event (precision guard below; one per such point) instead of returning NaN colours itself. That range is
 * [2^64, 2^76): the fp16-pair kernels scale a point's activations by 2^-60 at most and carry them as fp16 numbers, so
 * neither kernel represents a trunk output of 2^76 or more (tests/test_view_fold.py works inside [2^68, 2^76): a folded
 * network's gain is below 2^64, and one the tests can call eligible before equalisation has a gain of at most 2^60).
 * nerf_set_view_fold: on (default) / off for the following launches of this context; results are valid either way.
 * nerf_view_fold_status: *folded = 1 if deterministic fp16-pair inference launches of `slot` use the fold (0: not eligible, no
 * view branch, or switched off). Synchronises the device. */
int nerf_set_view_fold(nerf_ctx* ctx, int on);
/* Per-ray view bias: in a folded render of ray records with a multiple of 32 samples per ray (nerf_render_rays /
 * nerf_render_frame, with or without an occupancy grid) what the view layer adds for gamma(dir) is formed once per ray -
 * b_vf + W_v[:, W:] gamma(dir), accumulated in fp64, rounded once - and the kernel neither encodes the direction per point nor
 * runs its chunk. Without a grid every wavefront of 32 points lies on one ray and takes its ray's row through LDS; with a grid
 * each point reads its own ray's row, the same values: an all-occupied grid still gives the dense render bit for bit. sigma is bit for bit the folded kernel's; the colours differ by the rounding of that term.
 * on (default) / off for the following launches of this context; every other launch is what it was. */
int nerf_set_ray_view_bias(nerf_ctx* ctx, int on);
/* Tile schedule of the inference MLP launches. A launch is one persistent workgroup per compute unit over equal tiles of 128
 * points. NERF_TILES_STATIC: workgroup b runs tiles b, b + grid, ... - equal shares, and the launch ends with the slowest
 * XCD (the eight dies hold clocks a few per cent apart under this load). NERF_TILES_CLAIMED (default): workgroups take
 * batches of tiles from a counter in device memory, a decreasing sequence of sizes down to single tiles, so that all of them
 * end within about one tile of each other. Which workgroup runs a tile changes no value: every output is bit for bit the
 * same under both. Training passes and launches of one tile per workgroup or fewer are static always. For the following
 * launches of this context. */
#define NERF_TILES_STATIC 0
#define NERF_TILES_CLAIMED 1
int nerf_set_tile_schedule(nerf_ctx* ctx, int schedule);
int nerf_view_fold_status(nerf_ctx* ctx, int slot, int* folded);
/* NERF_PRECISION_F16X2 chooses a layer's per-point output scale from an a-priori bound (largest row sum of |W| x
 * largest |input| + largest |bias|). A bound 2^12 or more above a point's real outputs starts to cost low-order
 * bits; each such (wavefront, layer) occurrence is counted, never silent. Synchronises the device; `reset` zeroes the
 * counters. The figure is the sum of two counters: the rendering calls' and the training step's (kept apart so that each
 * side's guard sees only its own events). 0 on every network trained or initialised like a NeRF; non-zero means: compare
 * with NERF_PRECISION_F32 on these weights (rows of large weights that cancel). */
int nerf_precision_status(nerf_ctx* ctx, int64_t* loose_bound_events, int reset);
/* Precision guard: how that counter reaches the caller without being asked for. The reference evaluates the network in
 * fp32 (nerf/nerf.py:57-111 under torch.float32, nerf.ipynb:76), so a loose bound must not pass silently:
 *   nerf_render_frame / nerf_render_shard   args->precision_guard: NERF_GUARD_OFF enqueue and return as before;
 *                        NERF_GUARD_REPORT synchronise the stream at the end and return NERF_W_PRECISION if events were
 *                        counted during the frame; NERF_GUARD_FALLBACK additionally render the range again with the fp32
 *                        kernel and return NERF_W_PRECISION_FALLBACK (the Python mirror's render() does this).
 *   nerf_render_rays     stays asynchronous; it enqueues a 4-byte copy of the counter to a pinned host mirror behind its
 *                        kernels. nerf_precision_peek reads the mirror WITHOUT synchronising (events of completed work that
 *                        have not been reported yet); nerf_precision_check synchronises `stream` first. Both mark what
 *                        they return as reported. The Python mirror peeks on entry of render_rays() and checks at the end
 *                        of batchify_rays(), which re-renders the chunks in fp32 when the check is positive.
 *   nerf_train_step      peeks on entry at ITS OWN counter (a frame rendered in between neither consumes a step's events nor
 *                        adds to them): if events of an earlier step have become visible the context's TRAINING switches
 *                        to the fp32 kernels from this step on (until nerf_set_precision is called again) and the call
 *                        returns NERF_W_PRECISION_FALLBACK once. nerf_precision_peek / _check report rendering's events only. */
#define NERF_GUARD_OFF 0
#define NERF_GUARD_REPORT 1
#define NERF_GUARD_FALLBACK 2
/* counts[0] = the counter above; counts[1..7] = the training step's backward-data kernel (gradients, scaled per point like
 * the activations): its (point, layer) events by the bound's overshoot, 2^12-13, 2^14-15, ..., 2^22-23, >= 2^24. These are
 * reported, not guarded: a ReLU-masked gradient vector is sparse, so its largest entry often lies far below the bound of
 * the product it came from - one event in four on the test networks - without any loss that matters: the error of a
 * layer's gradient stays 2^-22 of |W^T| max|dz| for that point (the norm-wise bound of any fp32 product), entries far below
 * the point's largest are what is coarser, and those are negligible in the sums over points the weight gradients are. The
 * gradient tests hold the fp16-pair path to the fp32 path's bars (tests/test_hip_parity.py: autograd parity, six decades of
 * ray errors, rows 2^20 apart). Synchronises the device. */
int nerf_precision_detail(nerf_ctx* ctx, int64_t* counts /*[host] [8]*/, int reset);
int nerf_precision_peek(nerf_ctx* ctx, int64_t* new_events);
int nerf_precision_check(nerf_ctx* ctx, void* stream, int64_t* new_events);

/* Weights ---------------------------------------------------------------------------
 * Replaces NeRF.__init__ + load_state_dict (nerf/nerf.py:9-55; checkpoint reload at
 * nerf.ipynb:927-935). `tensors` are host pointers to the state_dict entries in this
 * order, each exactly as PyTorch stores it (weight [out,in] row-major, bias [out]):
 *   pts_linears.0.weight, pts_linears.0.bias, ..., pts_linears.{D-1}.weight, .bias,
 *   views_linears.0.weight, views_linears.0.bias,
 *   then if use_viewdirs: feature_linear.{weight,bias}, alpha_linear.{weight,bias},
 *                         rgb_linear.{weight,bias}
 *        else:            output_linear.{weight,bias}
 * The weights are repacked once into the MFMA fragment stream the kernel consumes.
 */
int nerf_load_weights(nerf_ctx* ctx, int slot, const nerf_arch* arch,
                      const float* const* tensors /*[host]*/, int n_tensors);
/* Expected tensor count for an architecture (2*D + 2 + (use_viewdirs ? 6 : 2)). */
int nerf_num_weight_tensors(const nerf_arch* arch);

/* Stage entry points (each backs one reference callable) --------------------------- */

/* Embedder.embed / get_embedder (nerf/embedder.py:72-80, 82-116).
 * x [n,3] -> out [n, 3+6*multires]; multires == 0 is the i_embed == -1 identity. */
int nerf_embed(nerf_ctx* ctx, const float* x /*[dev]*/, int64_t n, int multires,
               float* out /*[dev]*/, void* stream);

/* NeRF.forward (nerf/nerf.py:57-111) on already-encoded rows
 * x [B, input_ch + input_ch_views] -> out [B, out_ch] where out_ch is 4 with viewdirs
 * and arch.output_ch without. */
int nerf_mlp_forward(nerf_ctx* ctx, int slot, const float* x /*[dev]*/, int64_t B,
                     float* out /*[dev]*/, void* stream);

/* run_network (nerf.ipynb:790-855) with embed_fn/embeddirs_fn = get_embedder(multires /
 * multires_views): pts [n_rays*n_samples,3], viewdirs [n_rays,3] (NULL when the model
 * does not use them) -> out [n_rays*n_samples, out_ch]. Encoding, the per-sample
 * broadcast of viewdirs and the MLP are fused; netchunk does not exist (results are
 * independent of it). */
int nerf_run_network(nerf_ctx* ctx, int slot, const float* pts /*[dev]*/,
                     const float* viewdirs /*[dev]*/, int64_t n_rays, int64_t n_samples,
                     float* out /*[dev]*/, void* stream);

/* raw2outputs (nerf.ipynb:254-349). raw [N,S,C] (C >= 4; channels 0-2 rgb logits,
 * 3 sigma), z_vals [N,S], rays_d [N,3], noise [N,S] or NULL (already scaled by
 * raw_noise_std - the caller owns the RNG). Any output pointer may be NULL. */
int nerf_raw2outputs(nerf_ctx* ctx, const float* raw /*[dev]*/, int C,
                     const float* z_vals /*[dev]*/, const float* rays_d /*[dev]*/,
                     const float* noise /*[dev]*/, int white_bkgd, int64_t N, int S,
                     float* rgb_map /*[dev] [N,3]*/, float* disp_map /*[dev] [N]*/,
                     float* acc_map /*[dev] [N]*/, float* weights /*[dev] [N,S]*/,
                     float* depth_map /*[dev] [N]*/, void* stream);

/* sample_pdf (nerf/nerf_helpers.py:372-439). bins [N,M], weights [N,M-1],
 * u [N,n_samples] or NULL for det=True (u = linspace(0,1,n_samples)) -> out [N,n_samples]. */
int nerf_sample_pdf(nerf_ctx* ctx, const float* bins /*[dev]*/, const float* weights /*[dev]*/,
                    const float* u /*[dev]*/, int64_t N, int M, int n_samples,
                    float* out /*[dev]*/, void* stream);

/* Stratified depths of render_rays (nerf.ipynb:418-444): z_vals [N, N_samples] from the near/far columns of
 * the ray record; lindisp samples uniformly in disparity; t_rand [N, N_samples] (or NULL) jitters every
 * sample inside its stratum (perturb > 0). */
int nerf_stratified_z(nerf_ctx* ctx, const float* rays /*[dev]*/, int ray_stride, int64_t N, int N_samples,
                      int lindisp, const float* t_rand /*[dev]*/, float* z_vals /*[dev]*/, void* stream);

/* The resampling stage of render_rays (nerf.ipynb:458-467, 486): z_vals_mid, sample_pdf on
 * weights[...,1:-1], then sort(cat[z_vals, z_samples]) and std(z_samples). u [N,n_samples] or NULL (det).
 * z_samples, z_merged [N, S+n_samples] and z_std [N] may each be NULL. */
int nerf_resample(nerf_ctx* ctx, const float* z_vals /*[dev] [N,S]*/, const float* weights /*[dev] [N,S]*/,
                  const float* u /*[dev]*/, int64_t N, int S, int n_samples, float* z_samples /*[dev]*/,
                  float* z_merged /*[dev]*/, float* z_std /*[dev]*/, void* stream);

/* The ray-chunk renderer ------------------------------------------------------------
 * render_rays (nerf.ipynb:359-492) for one chunk of rays, all stages on the device with
 * no host synchronisation: stratified depths -> encode+MLP (coarse) -> composite ->
 * sample_pdf -> merge/sort -> encode+MLP (fine) -> composite -> z_std.
 */
typedef struct nerf_render_args {
    const float* rays;          /* [dev] [N, ray_stride]: o(3) d(3) near far [viewdir(3)]
                                   exactly as render() packs it (nerf.ipynb:622-629)  */
    int64_t n_rays;
    int32_t ray_stride;         /* 8 or 11 (floats per ray)                            */
    int32_t N_samples;          /* S_c                                                 */
    int32_t N_importance;       /* S_i, 0 disables the fine pass                       */
    int32_t slot_coarse;        /* network_fn                                          */
    int32_t slot_fine;          /* network_fine, or -1 to reuse network_fn (:471)      */
    int32_t lindisp;
    int32_t white_bkgd;
    int32_t perturb;            /* perturb > 0: t_rand must be given; u_rand replaces
                                   the deterministic linspace (det = perturb == 0)     */
    const float* t_rand;        /* [dev] [N,S_c] uniforms for stratified jitter or NULL */
    const float* u_rand;        /* [dev] [N,S_i] uniforms for sample_pdf or NULL        */
    const float* noise0;        /* [dev] [N,S_c] sigma noise (scaled) coarse, or NULL   */
    const float* noise;         /* [dev] [N,S_c+S_i] sigma noise fine pass, or NULL     */
    /* outputs, any may be NULL */
    float* rgb_map;             /* [dev] [N,3] last pass                               */
    float* disp_map;            /* [dev] [N]                                           */
    float* acc_map;             /* [dev] [N]                                           */
    float* raw;                 /* [dev] [N,S_last,out_ch] (retraw)                    */
    float* rgb0;                /* [dev] [N,3] coarse pass (N_importance > 0)          */
    float* disp0;               /* [dev] [N]                                           */
    float* acc0;                /* [dev] [N]                                           */
    float* z_std;               /* [dev] [N]                                           */
    /* optional intermediates for stage-wise parity */
    float* z_vals_coarse;       /* [dev] [N,S_c]                                       */
    float* weights_coarse;      /* [dev] [N,S_c]                                       */
    float* z_samples;           /* [dev] [N,S_i]                                       */
    float* z_vals_fine;         /* [dev] [N,S_c+S_i]                                   */
    float* weights_fine;        /* [dev] [N,S_c+S_i]                                   */
    float* depth_map;           /* [dev] [N] last pass                                 */
    const float* z_vals_fine_in;/* [dev] [N,S_c+S_i] inject fine depths (skips sampling) */
    void* stream;
} nerf_render_args;

int nerf_render_rays(nerf_ctx* ctx, const nerf_render_args* args);

/* Ray generation ---------------------------------------------------
 * get_rays (nerf/nerf_helpers.py:222-296) + the packing done by render() (nerf.ipynb:596-629):
 * viewdir normalisation before the NDC warp and before the c2w_staticcam override, optional
 * ndc_rays (nerf_helpers.py:311-369, called with near = 1.0), near/far columns. Writes the
 * [n_pixels, 8|11] ray record for flat pixel indices [first_pixel, first_pixel + n_pixels) of the
 * H x W image (row-major, index = row*W + col), so a rank can generate only its own shard.
 */
typedef struct nerf_camera {
    int32_t H, W;
    float fx, fy, cx, cy;       /* K[0][0], K[1][1], K[0][2], K[1][2] as fp32 (what torch casts to) */
    float c2w[12];              /* camera-to-world [3,4] row-major                               */
    float c2w_static[12];       /* c2w_staticcam, used when has_static != 0                       */
    int32_t has_static;
    int32_t ndc;
    double ndc_focal;           /* K[0][0] as the Python float that ndc_rays receives             */
    float near, far;            /* columns 6 and 7                                                */
    int32_t use_viewdirs;       /* 11 columns instead of 8                                        */
} nerf_camera;

int nerf_generate_rays(nerf_ctx* ctx, const nerf_camera* cam, int64_t first_pixel, int64_t n_pixels,
                       float* rays /*[dev] [n_pixels, 8|11]*/, void* stream);

/* render(rays=(rays_o, rays_d), ...) - the form the training loop calls (nerf.ipynb:1258) - packs a caller-supplied batch:
 * viewdirs = rays_d / |rays_d| taken before the NDC warp (nerf.ipynb:600-614), optional ndc_rays(H, W, K[0][0], 1., ...)
 * (:616-619), near / far columns (:622-629) -> the [n, 8|11] ray record. Of `cam` only H, W, ndc, ndc_focal, near, far and
 * use_viewdirs are read. rays_o / rays_d are [n, >= 3] with row strides of o_stride / d_stride floats (so that the two
 * halves of a stacked record can be passed in place). One kernel instead of the six tensor operations of the reference. */
int nerf_pack_rays(nerf_ctx* ctx, const nerf_camera* cam, const float* rays_o /*[dev]*/, int o_stride,
                   const float* rays_d /*[dev]*/, int d_stride, int64_t n, float* rays /*[dev] [n, 8|11]*/, void* stream);

/* render() for one camera (nerf.ipynb:558-640) in a single call: ray generation for the flat pixel range
 * [first_pixel, first_pixel + n_pixels), the batchify_rays chunk loop and render_rays per chunk, all enqueued
 * on `stream` with no host synchronisation. Deterministic rendering only (perturb = 0, raw_noise_std = 0:
 * render_kwargs_test); outputs are [n_pixels, ...] in pixel order, optional ones may be NULL. */
typedef struct nerf_frame_args {
    nerf_camera cam;
    int64_t first_pixel, n_pixels;
    int64_t chunk;              /* rays per render_rays call; <= 0 means 32768 (the reference default)   */
    int32_t N_samples, N_importance;
    int32_t slot_coarse, slot_fine;
    int32_t lindisp, white_bkgd;
    float* rgb_map;             /* [dev] [n_pixels,3] */
    float* disp_map;            /* [dev] [n_pixels]   */
    float* acc_map;             /* [dev] [n_pixels]   */
    float* rgb0;                /* [dev] optional, N_importance > 0 */
    float* disp0;
    float* acc0;
    float* z_std;
    void* stream;
    int32_t precision_guard;    /* NERF_GUARD_* (see "Precision guard"); 0 = none: the call only enqueues  */
} nerf_frame_args;

int nerf_render_frame(nerf_ctx* ctx, const nerf_frame_args* args);

/* Multi-GPU frame rendering (the `render_sharded` entry of section 8b's export list).
 * The reference's nerf/ path is single-device; rays are independent and cost the same, so the flat [H*W] pixel index is
 * cut into `world` contiguous shards (the first n_total % world ranks get one pixel more) and every rank - one process
 * and one nerf_ctx per GPU - renders its shard with no data-path collective:
 *   nerf_shard_bounds   the partition rule: rank owns [*first_pixel, *first_pixel + *n_pixels)
 *   nerf_render_shard   nerf_render_frame for that range: `args->first_pixel / n_pixels` are ignored and the range of
 *                       (world, rank) is used; outputs are [n_pixels of the shard, ...]; the range is returned through
 *                       first_pixel / n_pixels (may be NULL). An empty shard (n_total < world) renders nothing.
 * The one exchange per frame - gathering rgb|disp|acc (20 B/ray) to rank 0 - belongs to the host's collective library
 * (RCCL ncclGather / torch.distributed.gather on the same stream; INTEGRATION.md shows both): this library links
 * libamdhip64 only. nerf_render_frame(first_pixel, n_pixels) itself is the C-level shard call for any other partition. */
int nerf_shard_bounds(int64_t n_total, int world, int rank, int64_t* first_pixel, int64_t* n_pixels);
int nerf_render_shard(nerf_ctx* ctx, const nerf_frame_args* args, int world, int rank, int64_t* first_pixel,
                      int64_t* n_pixels);

/* Image metrics -----------------------------------------------------
 * calculate_ssim (nerf/nerf_helpers.py:21-111): separable 11-tap Gaussian (sigma 1.5), zero padded,
 * on [H,W,3] images clamped to [0,max_val]; img2mse (nerf_helpers.py:8). Results are written to
 * device scalars: out[0] = mean SSIM, out[1] = MSE of the clamped images. */
int nerf_image_metrics(nerf_ctx* ctx, const float* img1 /*[dev] [H,W,3]*/, const float* img2 /*[dev]*/,
                       int H, int W, float max_val, float* out /*[dev] [2]*/, void* stream);

/* Training step -----------------------------------------------------
 * One iteration of the reference's training loop body (nerf.ipynb:1258-1282) for a batch of rays:
 *   render(rays, retraw=True, **render_kwargs_train) -> loss = img2mse(rgb, target) [+ img2mse(rgb0,
 *   target) when N_importance > 0] -> loss.backward() -> torch.optim.Adam step,
 * on the master fp32 copy of the weights that nerf_load_weights keeps on the device. Afterwards the
 * inference entry points see the updated weights. The caller owns the RNG (t_rand, u_rand, noise*, as in
 * nerf_render_args), the ray batching and the learning-rate schedule (nerf.ipynb:1278-1282).
 * Arithmetic: the forward pass, backward-data and the weight gradients follow nerf_set_precision (NERF_PRECISION_F16X2:
 * fp16-pair arithmetic, whose error is the fp32 kernels'; NERF_TRAIN_FORWARD=f32 / NERF_TRAIN_BWD=f32 / NERF_TRAIN_DW=f32 in
 * the environment keep fp32 for that stage); compositing, its backward, Adam and the master weights are fp32.
 */
typedef struct nerf_train_args {
    const float* rays;          /* [dev] [N, 8|11] as render() packs them                       */
    const float* target;        /* [dev] [N,3] target_s                                         */
    int64_t n_rays;
    int32_t ray_stride;
    int32_t N_samples, N_importance;
    int32_t slot_coarse, slot_fine;     /* slot_fine < 0 with N_importance > 0: both passes through slot_coarse (network_fine=None,
                                           nerf.ipynb:471); its gradient is the sum over the passes */
    int32_t lindisp, white_bkgd, perturb;
    const float* t_rand;        /* [dev] [N,S_c]      */
    const float* u_rand;        /* [dev] [N,S_i]      */
    const float* noise0;        /* [dev] [N,S_c]      */
    const float* noise;         /* [dev] [N,S_c+S_i]  */
    float lr, beta1, beta2, eps;        /* Adam; the reference uses betas (0.9, 0.999), eps 1e-8     */
    int32_t step;               /* 1-based optimizer step count (bias correction)               */
    int32_t apply_update;       /* 0: compute loss and gradients only                           */
    float* loss;                /* [dev] [2]: img_loss of the last pass, img_loss0 of the coarse pass */
    float* rgb_map;             /* [dev] [N,3] optional                                         */
    float* rgb0;                /* [dev] [N,3] optional                                         */
    void* stream;
    const float* z_vals_fine_in;/* [dev] [N,S_c+S_i] optional: the fine pass at THESE depths instead of the resampled ones (the
                                   resampling still runs; parity tests inject the reference's fine depths, as
                                   nerf_render_args::z_vals_fine_in does for rendering: sample_pdf is ill-conditioned where a
                                   bin's mass is tiny, and a depth that moves by 5e-4 turns the top-frequency columns of
                                   gamma(x) - hence layer 0's weight gradient - by a third of a radian)            */
    float* stats;               /* [dev] [5] optional: img_loss, img_loss0, loss = their sum, psnr = mse2psnr(img_loss), psnr0
                                   (nerf.ipynb:1262-1272, nerf_helpers.py:14) - what the loop body prints, without a tensor
                                   operation per number (entries 1 and 4 are 0 when N_importance = 0)            */
} nerf_train_args;

int nerf_train_step(nerf_ctx* ctx, const nerf_train_args* args);
/* Current master weights / last gradients of a slot, copied to host tensors in nerf_load_weights order. */
int nerf_get_weights(nerf_ctx* ctx, int slot, float* const* tensors /*[host]*/, int n_tensors);
int nerf_get_gradients(nerf_ctx* ctx, int slot, float* const* tensors /*[host]*/, int n_tensors);
/* torch.optim.Adam's per-parameter state (exp_avg, exp_avg_sq) of a slot, host tensors in nerf_load_weights order:
 * the 'optimizer_state_dict' of the reference's checkpoints (nerf.ipynb:1290-1299; reloaded at :925-932). */
int nerf_get_adam_state(nerf_ctx* ctx, int slot, float* const* exp_avg /*[host]*/, float* const* exp_avg_sq /*[host]*/,
                        int n_tensors);
int nerf_set_adam_state(nerf_ctx* ctx, int slot, const float* const* exp_avg /*[host]*/,
                        const float* const* exp_avg_sq /*[host]*/, int n_tensors);

/* Differentiable rendering: loss.backward() through the training kernels ---------------------------------------------
 * nerf_train_step with the loss left to the caller. nerf_train_forward renders a batch as render(rays, retraw=True,
 * **render_kwargs_train) does (the same kernels and random numbers as nerf_train_step) and keeps a TAPE: the activations,
 * ReLU masks and maxima of both passes, their depths and the inputs the backward pass re-reads, in an arena the context owns
 * (grow-only, apart from the render workspace). nerf_train_backward takes the caller's gradients on the outputs (NULL =
 * zero), runs raw2outputs' backward of both passes and the backward pass of nerf_train_step, and ADDS the weight gradients
 * into those nerf_get_gradients reads (nerf_zero_grad clears them): loss.backward() with .grad accumulating. It consumes
 * the tape. One tape is current per context; it stops being current after another nerf_train_forward, nerf_train_step,
 * nerf_adam_step or nerf_load_weights, and a backward on it then returns NERF_E_STATE. With only d_rgb / d_rgb0 given the
 * gradients are nerf_train_step's for the same upstream values, bit for bit. nerf_adam_step is nerf_train_step's update
 * (and refresh of the derived weight copies) on its own. The precision guard acts in nerf_train_forward as it does in
 * nerf_train_step. Both argument structs start with struct_size = sizeof(the struct), which the library checks. */
typedef struct nerf_train_forward_args {
    size_t struct_size;         /* sizeof(nerf_train_forward_args)                                           */
    const float* rays;          /* [dev] [N, 8|11] as render() packs them                                    */
    int64_t n_rays;
    int32_t ray_stride;
    int32_t N_samples, N_importance;
    int32_t slot_coarse, slot_fine;     /* as nerf_train_args                                                 */
    int32_t lindisp, white_bkgd, perturb;
    const float* t_rand;        /* [dev] [N,S_c]      (the caller's RNG, as nerf_train_args)                 */
    const float* u_rand;        /* [dev] [N,S_i]      */
    const float* noise0;        /* [dev] [N,S_c]      */
    const float* noise;         /* [dev] [N,S_c+S_i]  */
    const float* z_vals_fine_in;/* [dev] [N,S_c+S_i] optional, as nerf_train_args                             */
    float* rgb_map;             /* [dev] [N,3] outputs of the last pass, each optional                        */
    float* disp_map;            /* [dev] [N]   */
    float* acc_map;             /* [dev] [N]   */
    float* rgb0;                /* [dev] [N,3] outputs of the coarse pass (N_importance > 0), optional        */
    float* disp0;               /* [dev] [N]   */
    float* acc0;                /* [dev] [N]   */
    float* raw;                 /* [dev] [N, S_last, C_last] optional: the last pass's network output (retraw) */
    void* stream;
    uint64_t* tape;             /* [host] out: the tape's id                                                  */
} nerf_train_forward_args;

typedef struct nerf_train_backward_args {
    size_t struct_size;         /* sizeof(nerf_train_backward_args)                                          */
    uint64_t tape;              /* what nerf_train_forward returned                                          */
    const float* d_rgb;         /* [dev] [N,3] dL/d rgb_map; every gradient is optional (NULL = zero)        */
    const float* d_disp;        /* [dev] [N]   */
    const float* d_acc;         /* [dev] [N]   */
    const float* d_rgb0;        /* [dev] [N,3] */
    const float* d_disp0;       /* [dev] [N]   */
    const float* d_acc0;        /* [dev] [N]   */
    const float* d_raw;         /* [dev] [N, S_last, C_last] dL/d raw of the last pass                       */
    void* stream;
} nerf_train_backward_args;

int nerf_train_forward(nerf_ctx* ctx, const nerf_train_forward_args* args);
int nerf_train_backward(nerf_ctx* ctx, const nerf_train_backward_args* args);
/* Zeroes a slot's gradients (optimizer.zero_grad()). */
int nerf_zero_grad(nerf_ctx* ctx, int slot, void* stream);
/* optimizer.step(): torch.optim.Adam over the n (1 or 2, distinct) slots, as nerf_train_step applies it after its backward
 * pass; step is the 1-based step count. */
int nerf_adam_step(nerf_ctx* ctx, const int32_t* slots /*[host] [n]*/, int n, float lr, float beta1, float beta2, float eps,
                   int step, void* stream);

/* Measurement hooks ------------------------------------------------------------------
 * Accumulated device time of the dominant kernel (the fused encode+MLP kernel),
 * measured with HIP events recorded on the launch stream around every launch while
 * profiling is enabled. nerf_profile_read synchronises those events. */
int nerf_profile_enable(nerf_ctx* ctx, int on);
int nerf_profile_read(nerf_ctx* ctx, double* mlp_ms, int64_t* mlp_launches,
                      int64_t* mlp_points, int reset);

/* The same for the training step's kernels (HIP events on the step's stream while profiling is enabled), summed by kind:
 * [0] the forward passes' fused launches, [1] the backward-data launches, [2] the hidden-width weight-gradient launches
 * with their slice reductions, [3] the other weight gradients. ms / launches / points are [4] arrays (NULL = not wanted). */
int nerf_profile_read_train(nerf_ctx* ctx, double* ms /*[host] [4]*/, int64_t* launches /*[host] [4]*/,
                            int64_t* points /*[host] [4]*/, int reset);

/* Bytes of device workspace currently held by the context. */
int64_t nerf_workspace_bytes(nerf_ctx* ctx);

/* Mesh extraction -------------------------------------------------------------------------------
 * gen_mesh.marching_cubes (plenoctree/nerf_sh/gen_mesh.py:88-129) on the device, in two calls.
 *
 * nerf_density_grid: sigma = relu(raw[..., 3]) (nerf.ipynb:291) of network `slot` on the regular lattice of
 * reso[0] x reso[1] x reso[2] nodes spanning [c1, c2] (gen_mesh.py:104-119). Node (i, j, k) is point
 * n = (i * reso[1] + j) * reso[2] + k of sigma [dev] [X, Y, Z] (C order, x slowest); its coordinate on axis a is
 * np.linspace(c1[a], c2[a], reso[a], dtype=np.float32)[i]: fp64 i * ((c2 - c1) / (reso - 1)) + c1 with two roundings (no
 * fma), the last node exactly c2, then rounded to fp32. The fused encode+MLP kernel evaluates the lattice in place of a
 * point buffer (no point is read, no view direction: sigma does not depend on it) and writes one float per node (NaN
 * propagates as through F.relu). The result equals relu(nerf_run_network(...)[..., 3]) on the same points in the same
 * order, bit for bit, in either arithmetic (nerf_set_render_precision). precision_guard as for nerf_render_frame:
 * NERF_GUARD_FALLBACK evaluates the lattice again with the fp32 kernel when the fp16-pair kernel's scale bound was loose.
 * reso[a] must be in [2, 1024], c2[a] > c1[a], both finite.
 *
 * nerf_marching_cubes: the isosurface v = iso of any device volume [X, Y, Z] of fp32 (mcubes.marching_cubes,
 * gen_mesh.py:124), every axis in [2, 1024]. Conventions:
 *   - a node is INSIDE iff v >= iso (NaN is outside).
 *   - one vertex per lattice edge whose ends classify differently (welded: shared by every triangle that uses the edge).
 *     With a the value at the edge's lower-index end and b at the other, t = (iso - a) / (b - a) in fp32 (0.5 when t is
 *     not finite: a NaN or infinite end); the vertex is (i, j, k) with t added (fp32) on the edge's axis, in INDEX
 *     coordinates as mcubes returns them.
 *   - vertex order: by edge key 3 * ((i * Y + j) * Z + k) + axis (axis 0, 1, 2 = x, y, z); triangles: by cell (C order over
 *     [X-1, Y-1, Z-1]), then in table order within the cell. No atomics on the output path: two calls return identical
 *     arrays.
 *   - winding: the right-hand normal of every triangle points OUT of the region v >= iso, so a closed surface around an
 *     inside region has positive signed volume. Ambiguous faces separate the inside corners; the two cells that share a
 *     face draw the same segments on it, so a surface that stays inside the lattice is closed and every edge has exactly
 *     two triangles.
 *   - vertices [dev] [V, 3] fp32, triangles [dev] [T, 3] int64 vertex ids. With both output pointers NULL the call only
 *     counts: *n_vertices, *n_triangles are exact. If a capacity is too small nothing is written, the call returns
 *     NERF_E_INVALID and *n_vertices / *n_triangles report what is needed.
 *   - the call synchronises `stream` (the counts decide the writes); its scratch is the context's workspace
 *     (nerf_workspace_bytes includes it: 2 bytes per node and a few per 2048 nodes). */
typedef struct nerf_grid_args {
    double c1[3], c2[3];        /* lattice corners (the Python floats gen_mesh passes)                           */
    int32_t reso[3];            /* nodes per axis                                                                */
    int32_t slot;               /* network (coarse or fine, gen_mesh's --coarse)                                 */
    float* sigma;               /* [dev] [X, Y, Z]                                                               */
    void* stream;
    int32_t precision_guard;    /* NERF_GUARD_*                                                                  */
} nerf_grid_args;

int nerf_density_grid(nerf_ctx* ctx, const nerf_grid_args* args);

typedef struct nerf_mc_args {
    const float* volume;        /* [dev] [X, Y, Z]                                                               */
    int32_t reso[3];            /* X, Y, Z                                                                       */
    float iso;
    float* vertices;            /* [dev] [vertex_capacity, 3] or NULL (count only)                               */
    int64_t vertex_capacity;
    int64_t* triangles;         /* [dev] [triangle_capacity, 3] or NULL (count only)                             */
    int64_t triangle_capacity;
    int64_t* n_vertices;        /* [host] out                                                                    */
    int64_t* n_triangles;       /* [host] out                                                                    */
    void* stream;
} nerf_mc_args;

int nerf_marching_cubes(nerf_ctx* ctx, const nerf_mc_args* args);

/* Occupancy grid --------------------------------------------------------------------------------
 * Rendering that skips the network at samples in empty space. A grid is the axis-aligned box [c1, c2] cut into
 * (X-1) x (Y-1) x (Z-1) CELLS by the nodes of the lattice nerf_density_grid evaluates (reso = nodes per axis), one bit per
 * cell. It is a snapshot of the networks it was built from: nothing invalidates it when the weights change.
 *
 * Rendering with a grid is the reference's render_rays with a masked network, in the coarse pass (S = N_samples) and in
 * the fine pass (S = N_samples + N_importance) alike:
 *     keep[n, i] = (i == S - 1) or occupied(cell(pts[n, i])) or (pts[n, i] outside the box and outside == NERF_OCC_EVALUATE)
 *     raw[n, i]  = network(pts[n, i], viewdir[n]) if keep[n, i], else 0 in every channel
 * and everything else unchanged (raw2outputs, sample_pdf on the masked coarse weights, the returned raw shows the zeros).
 * Two rules are not optional:
 *   - the LAST sample of every ray is always evaluated: its dists is 1e10 (nerf.ipynb:300), so skipping it where sigma is a
 *     hair above zero would turn a whole pixel from the scene's colour to the background;
 *   - skipped samples are ZEROS in raw, not absent: relu(0) = 0, alpha = 0, weight = 0, as for any empty sample. Where no
 *     skipped sample has sigma > 0 the masked render equals the dense one.
 * The cell rule: pts = rays_o + rays_d * z, product and sum each rounded to fp32. With c1, c2 rounded to fp32 and
 * cell = (c2 - c1) / (reso - 1) (fp32, each operation rounded), a point is inside the box iff c1 <= p <= c2 on every axis,
 * and its cell index on an axis is min(floor((p - c1) / cell), reso - 2), subtraction and division each rounded to fp32:
 * points on an upper face belong to the last cell. A NaN or infinite position counts as occupied (the reference's NaN comes
 * out). A cell is occupied when, in any of the n_lattices sigma lattices ([dev] [X, Y, Z] as nerf_density_grid writes them),
 * sigma at any of its 8 corner nodes is > threshold or NaN, or when its byte of cell_mask ([dev] [X-1, Y-1, Z-1], optional)
 * is non-zero; the set is then grown `dilate` times by one cell in all 26 directions. The lattice only samples the field: a
 * grid is not guaranteed conservative.
 *
 * The kept points of a pass are listed in increasing order by three stream-ordered launches (no atomics, no workgroup waits
 * for another), and the fused kernel runs over that list: no host synchronisation inside a frame, and two renders of the
 * same input are bit-identical. In NERF_PRECISION_F32 a kept point's raw row is bit-identical to the dense render's.
 * nerf_render_rays_occ / nerf_render_frame_occ are nerf_render_rays / nerf_render_frame with a grid (NULL: the plain call);
 * the frame's precision guard re-renders with the grid too. Counters of evaluated / total points accumulate on the device
 * and follow every call to a pinned host mirror; nerf_occupancy_stats waits for the device and reads them.
 * nerf_occupancy_create synchronises `stream` (it returns with the count of occupied cells known). reso[a] in [2, 1024].
 * A grid belongs to the context it was created on: use it with that context only, and destroy it before the context.
 * The taped calls (nerf_train_forward / nerf_train_backward) and nerf_render_shard take no grid.
 *
 * Training with a grid: nerf_train_step_occ is nerf_train_step - the reference's loop body, nerf.ipynb:1258-1282 - with the
 * network query of both passes replaced by the masked query above. Everything else is the dense step: sample_pdf on the
 * (masked) coarse weights, both MSE terms, Adam, z_vals_fine_in, perturb, lindisp, white_bkgd; nerf_train_args is unchanged.
 *   - Which samples are kept: the rule above, by the same device function - `outside` as the grid says, a non-finite
 *     position kept, the last sample of every ray always kept.
 *   - Skipped samples have a raw row of zeros, and their alpha is EXACTLY 0 even with sigma noise (noise0 / noise): the
 *     noise is not applied to a skipped sample (relu(0 + noise) would be positive at half of all empty samples, and the
 *     step would train against fog). Rendering calls keep their behaviour: there the caller's noise reaches every sample.
 *   - Gradients: a skipped sample sends no gradient to any parameter; a kept sample sends exactly what the dense step
 *     would send given the same raw everywhere. A cell wrongly called empty therefore receives no gradient until a
 *     refresh finds density there.
 *   - Statistics: both passes are counted in the grid's evaluated / total counters like rendering passes.
 *   - slot_fine < 0 with N_importance > 0 (one network, two passes, gradients summed), networks without view directions
 *     and networks narrower than 256 work as in nerf_train_step.
 *   - Determinism: the same batch, grid and weights give the same bits in either arithmetic. In NERF_PRECISION_F32 a kept
 *     point's forward values do not depend on where it stands in the list; in NERF_PRECISION_F16X2 the per-wavefront
 *     input scale makes the last bits depend on which 32 kept points share a wavefront. A grid that keeps every
 *     sample gives nerf_train_step's bits.
 *   - The kept count of each pass crosses to the host (one stream synchronisation per pass): the backward and
 *     weight-gradient launches are sized by it.
 * A NULL grid or one of another context is NERF_E_INVALID.
 * nerf_occupancy_refresh rebuilds the cells of an existing grid in place from new lattices / a new mask (threshold, dilate
 * and outside as given): same handle, same bit table, the statistics counters untouched, the occupied count updated. Box and
 * resolution must be the grid's own (NERF_E_INVALID otherwise). It synchronises `stream`; work on other streams that reads
 * the grid must have finished. */
#define NERF_OCC_EVALUATE 0       /* points outside the box are evaluated                                          */
#define NERF_OCC_EMPTY 1          /* points outside the box are skipped                                            */
typedef struct nerf_occupancy nerf_occupancy;
typedef struct nerf_occupancy_args {
    double c1[3], c2[3];        /* box corners                                                                   */
    int32_t reso[3];            /* nodes per axis (cells = reso - 1)                                             */
    int32_t n_lattices;         /* 0..8 (0 only with cell_mask)                                                  */
    const float* const* sigma;  /* [host] n_lattices pointers to [dev] [X, Y, Z]                                 */
    const uint8_t* cell_mask;   /* [dev] [X-1, Y-1, Z-1] or NULL                                                 */
    float threshold;
    int32_t dilate;             /* >= 0                                                                          */
    int32_t outside;            /* NERF_OCC_*                                                                    */
    void* stream;
} nerf_occupancy_args;

int nerf_occupancy_create(nerf_ctx* ctx, const nerf_occupancy_args* args, nerf_occupancy** out);
void nerf_occupancy_destroy(nerf_occupancy* occ);
/* the cells as bytes (0 / 1) into mask [dev] [X-1, Y-1, Z-1] (NULL: not wanted) and their count */
int nerf_occupancy_cells(const nerf_occupancy* occ, uint8_t* mask, int64_t* n_occupied /*[host]*/, void* stream);
/* points the network evaluated / points of the passes rendered with this grid since the last reset */
int nerf_occupancy_stats(nerf_occupancy* occ, int64_t* evaluated /*[host]*/, int64_t* total /*[host]*/, int reset);
int nerf_render_rays_occ(nerf_ctx* ctx, const nerf_render_args* args, const nerf_occupancy* occ);
int nerf_render_frame_occ(nerf_ctx* ctx, const nerf_frame_args* args, const nerf_occupancy* occ);
int nerf_train_step_occ(nerf_ctx* ctx, const nerf_train_args* args, nerf_occupancy* occ);
int nerf_occupancy_refresh(nerf_occupancy* occ, const nerf_occupancy_args* args);

/* Sparse voxel grid ------------------------------------------------------------------------------
 * A Plenoxels grid (svox2.SparseGrid, forward side): X x Y x Z nodes, a density and 3 * basis_dim spherical-harmonic colour
 * coefficients at every KEPT node, rendered by trilinear ray marching without any network.
 *   links        [dev] int32 [X, Y, Z], C order: >= 0 = row of the data arrays, ANY negative value = empty node. Values < -1
 *                carry no meaning here (the reference stores skip distances in them; they are not trusted).
 *   density_data [dev] float [capacity, 1]
 *   sh_data      [dev] float [capacity, 3 * basis_dim], channel-major: [r_0 .. r_(B-1), g_0 .., b_0 ..]
 * The three arrays are BORROWED: the grid keeps the pointers, the caller keeps the memory alive and unchanged in size until
 * nerf_grid_destroy. Values may change between calls (stream order) - nerf_grid_optim_step is how training changes them: the
 * grid holds const pointers, the optimiser writes through the caller's own non-const pointers to the same memory, and the next
 * call on the grid reads the new values. After a change of `links` call nerf_grid_accelerate
 * again or nerf_grid_drop_skip - skip data made from other links is wrong (skip data depends on `links` alone: it stays
 * valid across optimiser steps). nerf_grid_create checks every link against
 * `capacity` on the device and synchronises `stream`; as a second line the kernels read a link >= capacity as empty.
 * Geometry: the grid covers center -+ radius; node i of axis a sits at the voxel centre
 * center - radius + (i + 0.5) * 2 radius / reso (grid coordinate i; the box is [-0.5, reso - 0.5]).
 *
 * Rendering (nerf_grid_render_rays / nerf_grid_render_image) is trace_ray_cuvol of the reference with the ray set-up and
 * the operation order of its PyTorch statement (svox2.py _volume_render_gradcheck_lerp), fp32, no fused multiply-adds:
 *   o = offset + origin * scaling (grid coordinates);  v = dir / |dir| (unit world direction, also the SH argument);
 *   d = v * scaling;  delta_scale = 1 / |d|;  d *= delta_scale;  tmin / tmax from the box with d == 0 axes left out,
 *   tmin = max(tmin, near_clip);  a ray with not (tmin <= tmax) returns the background and log_transmit 0.
 *   t = tmin; while t <= tmax: p = clamp(o + t d, 0, reso - 1); l = min(int(p), reso - 2); w = p - l;
 *     sigma = trilinear over the 8 corners (z, then y, then x; empty corner = 0);
 *     if sigma > sigma_thresh: c_k likewise; rgb = max(0, sum_k c_k Y_k(v) + 0.5); a = ((-step_size) sigma) delta_scale;
 *       out += exp(log_T) (1 - exp(a)) rgb; log_T += a; if exp(log_T) < stop_thresh: log_T = -1e3, stop
 *     t += step_size                       (accumulated in fp32, one addition per sample, also across skipped stretches)
 *   out += exp(log_T) background_brightness
 * Two renders of the same input are bit-identical, and so are a render with and without skip data.
 * Termination is unconditional. A ray whose set-up is not finite - a zero direction, a NaN or an infinity in origin or
 * direction - is a miss: background, log_transmit 0, nothing marched. The march leaves a ray as soon as t + step_size does not
 * exceed t in fp32 (t so large that step_size is below half an ulp: nothing further can be sampled), so every pass of the loop
 * advances t, and step_size >= 1e-3 is required. At most 2^26 rays, pixels, points or nodes per call (NERF_E_INVALID beyond).
 * nerf_grid_accelerate builds the skip data on the device (its own array, `links` is never written): per base cell the
 * Chebyshev distance, capped at 31 cells, to the nearest cell with a kept corner (stored value v = distance + 1, 0 = a corner
 * of the cell is kept). A ray at a sample t0 in a cell of value v > 0 skips that sample and every following sample whose
 * accumulated t satisfies t - t0 <= v - 1 - 1/16, without loading anything: a step moves every coordinate by at most the step
 * in t, so none of them can have a kept node among its 8 corners, and since t is accumulated by the same additions the sample
 * lattice of the ray is unchanged. The 1/16 covers the rounding of o + t d, which holds while |o| and |t| stay below 2^17 grid
 * units; a ray beyond that range is marched without the skip data.
 * A grid belongs to the context it was created on; destroy it before the context. */
typedef struct nerf_sparse_grid nerf_sparse_grid;
typedef struct nerf_sparse_grid_desc {
    size_t struct_size;         /* sizeof(nerf_sparse_grid_desc), checked                                           */
    int32_t reso[3];            /* nodes per axis, each in [2, 1024]                                                */
    int32_t basis_dim;          /* 1, 4 or 9 (spherical harmonics of degree 0, 1, 2)                                */
    float radius[3];            /* > 0                                                                              */
    float center[3];
    int64_t capacity;           /* rows of density_data / sh_data, >= 0                                             */
    const int32_t* links;       /* [dev] [X, Y, Z]                                                                  */
    const float* density_data;  /* [dev] [capacity, 1]          (may be NULL when capacity == 0)                    */
    const float* sh_data;       /* [dev] [capacity, 3 * basis_dim]                                                  */
    void* stream;
} nerf_sparse_grid_desc;

typedef struct nerf_grid_render_options {      /* svox2.RenderOptions as far as the forward cuvol kernel reads it     */
    size_t struct_size;
    float step_size;            /* 0.5; in voxels, >= 1e-3                                                            */
    float sigma_thresh;         /* 1e-10                                                                            */
    float stop_thresh;          /* 1e-7                                                                             */
    float background_brightness; /* 1.0                                                                             */
    float near_clip;            /* 0.0                                                                              */
    int32_t last_sample_opaque; /* must be 0 (not built)                                                            */
    int32_t randomize;          /* must be 0 (not built)                                                            */
} nerf_grid_render_options;

/* The NDC warp of forward-facing scenes (svox2.utils.convert_to_ndc with near = 1, then the normalisation that its two
 * callers, Camera.gen_rays and LLFFDataset.gen_rays, apply). rays_to_ndc(cx, cy, o, d), fp32, every operation rounded on its
 * own, true divisions, a correctly rounded root, in this order:
 *     t  = (1 - o.z) / d.z
 *     o  = o + t * d                                    (a product, then a sum: no fused multiply-add)
 *     o' = (cx * (o.x / o.z),  cy * (o.y / o.z),  1 - 2 / o.z)
 *     d' = (cx * (d.x / d.z - o.x / o.z),  cy * (d.y / d.z - o.y / o.z),  2 / o.z)
 *     n  = sqrt(fma(d'.z, d'.z, fma(d'.y, d'.y, d'.x * d'.x)))          (the fma chain of torch.norm's vectorised CPU sum)
 *     d' = d' / n
 * (cx, cy) are the ndc_coeffs (2 fx / width, 2 fy / height of the full-resolution images). Non-finite results (d.z == 0,
 * o.z == 0) are passed on as they come: every marching kernel treats a ray whose set-up is not finite as a miss. This is
 * the warp of svox2's Python path, whose rays its checkpoints were trained on; its CUDA world2ndc (another order, an fma)
 * is not built. Three callers: the camera below, nerf_grid_dataset_batch, and nerf_grid_rays_to_ndc for a caller's own rays. */
typedef struct nerf_grid_camera {              /* svox2.Camera. c2w is OpenCV: x right, y down, z forward             */
    size_t struct_size;         /* 104 (96 before ndc_coeffs was added: hosts built against that header are refused)  */
    float c2w[12];              /* [3, 4] row-major                                                                 */
    double fx, fy, cx, cy;      /* pixel (x, y) looks along ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)           */
    int32_t width, height;
    float ndc_coeffs[2];        /* both > 0 (and finite): the pixel's ray, rounded to fp32, goes through rays_to_ndc;
                                   ndc_coeffs[0] <= 0 (a zeroed tail, svox2's (-1, -1)): no NDC. NaN, infinity, or a
                                   positive [0] with [1] <= 0 is NERF_E_INVALID                                     */
} nerf_grid_camera;

typedef struct nerf_grid_render_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]       (nerf_grid_render_rays only)                             */
    const float* dirs;          /* [dev] [n_rays, 3], need not be unit                                              */
    int64_t n_rays;             /* nerf_grid_render_image: ignored, width * height rays in row-major pixel order     */
    float* rgb;                 /* [dev] [n_rays, 3]                                                                */
    float* log_transmit;        /* [dev] [n_rays] or NULL                                                           */
    unsigned long long* counters; /* [dev] [2] or NULL: += samples whose links were loaded, samples shaded (an instrumented launch
                                     with atomics; leave NULL in timed and in reproducible work)                    */
    int32_t use_skip;           /* 1: use the skip data if nerf_grid_accelerate made it; 0: plain march              */
    void* stream;
} nerf_grid_render_args;

typedef struct nerf_grid_sample_args {
    size_t struct_size;
    const float* points;        /* [dev] [n, 3] world coordinates, or grid coordinates with grid_coords              */
    int64_t n;
    int32_t grid_coords;
    int32_t want_colors;
    float* density;             /* [dev] [n, 1]                                                                     */
    float* sh;                  /* [dev] [n, 3 * basis_dim]; may be NULL without want_colors                         */
    void* stream;
} nerf_grid_sample_args;

int nerf_grid_create(nerf_ctx* ctx, const nerf_sparse_grid_desc* desc, nerf_sparse_grid** out);
void nerf_grid_destroy(nerf_sparse_grid* grid);
int nerf_grid_render_rays(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_render_args* args);
/* the rays of `cam` made on the device in fp64 and rounded to fp32 (svox2 Camera.gen_rays): one call per frame */
int nerf_grid_render_image(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
                           const nerf_grid_render_args* args);
/* those rays themselves: origins, dirs [dev] [height * width, 3] */
int nerf_grid_gen_rays(nerf_ctx* ctx, const nerf_grid_camera* cam, float* origins, float* dirs, void* stream);

/* rays_to_ndc (above) on a caller's rays, one lane per ray: origins_out / dirs_out [dev] [n, 3] from origins / dirs [dev]
 * [n, 3]. An output may be the very pointer of its input (each lane reads its ray before it writes it); any other overlap is
 * not allowed. 0 <= n <= 2^26, ndc_coeffs both positive and finite. Stream-ordered, allocates and synchronises nothing. */
typedef struct nerf_grid_rays_to_ndc_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n, 3]                                                                     */
    const float* dirs;          /* [dev] [n, 3], dirs need not be unit                                              */
    int64_t n;
    float ndc_coeffs[2];
    float* origins_out;         /* [dev] [n, 3]                                                                     */
    float* dirs_out;            /* [dev] [n, 3], unit                                                               */
    void* stream;
} nerf_grid_rays_to_ndc_args;

int nerf_grid_rays_to_ndc(nerf_ctx* ctx, const nerf_grid_rays_to_ndc_args* args);
/* svox2 SparseGrid.sample: trilinear, border padding, align_corners = False */
int nerf_grid_sample(nerf_sparse_grid* grid, const nerf_grid_sample_args* args);
int nerf_grid_accelerate(nerf_sparse_grid* grid, void* stream);
int nerf_grid_drop_skip(nerf_sparse_grid* grid);      /* waits for the device, frees the skip data                    */
int nerf_grid_has_skip(const nerf_sparse_grid* grid); /* 1 / 0                                                        */
/* Baking: rows [row0, row0 + m) of sh_out [., 3 * basis_dim] from network outputs raw [dev] [m, n_dirs, 4]:
 * sh_out[row0 + i, c * basis_dim + k] = sum_j P[k, j] * (sigmoid(raw[i, j, c]) - 0.5), fp32, the sum in order of j with
 * product and sum each rounded. P [dev] [basis_dim, n_dirs] (staged in LDS); basis_dim * n_dirs <= 4096. */
typedef struct nerf_grid_project_args {
    size_t struct_size;
    const float* raw;
    int64_t m;
    int32_t n_dirs;
    int32_t basis_dim;
    const float* P;
    float* sh_out;
    int64_t row0;
    void* stream;
} nerf_grid_project_args;
int nerf_grid_project_sh(nerf_ctx* ctx, const nerf_grid_project_args* args);

/* Sparse voxel grid: training ---------------------------------------------------------------------
 * The optimising half of svox2.SparseGrid: the fused render + MSE backward (volume_render_cuvol_fused without background
 * layers), the total-variation gradient over a range of cells (tv_grad_sparse_kernel) and the masked RMSProp / SGD step.
 * All three are stream-ordered and synchronise nothing. Gradients ACCUMULATE: the caller zeroes grad_density [capacity, 1],
 * grad_sh [capacity, 3 * basis_dim] and mask [capacity] (bytes) when a new step begins.
 *
 * nerf_grid_fused_backward renders n_rays rays exactly as nerf_grid_render_rays does - rgb_out (and log_transmit) are
 * bit-identical to that call's, with and without skip data - and adds the gradients of
 *   loss = mean over rays and channels of (rgb_out - rgb_gt)^2
 * with respect to density_data and sh_data. Every ray is marched a second time over the same sample lattice (the same fp32
 * additions of t, the same sigma_thresh and stop rules, the same skip data); fp32, each operation rounded, in this order -
 * except `remaining`, what the samples still to come add to the colour: it is the difference of two nearly equal sums, whose
 * fp32 rounding (6e-8 of the colour) would be a relative 1e-3 of the small density gradients behind a bright sample, so it is
 * carried in fp64:
 *   g_c = (rgb_c - gt_c) * (2 / (3 n_rays))
 *   remaining_c = the fp64 sum of the exact products weight * max(0, raw_c) of all shaded samples, plus exp(log_T) *
 *                 background_brightness: rgb_c once more, without the rounding of its fp32 sum
 *   at every shaded sample (sigma > sigma_thresh), with a, weight, log_T as in the render and raw_c = sum_k c_k Y_k + 0.5:
 *     dot = (max(0, raw_0) g_0 + max(0, raw_1) g_1) + max(0, raw_2) g_2
 *     remaining_c -= weight * max(0, raw_c)  (fp64, exact products);  accum = fp32(sum_c remaining_c g_c)  (svox2's accum)
 *     d_sigma = (step_size * delta_scale) * (exp(log_T after the sample) * dot - accum)
 *     d_coef(c, k) = (weight * Y_k) * g_c   where raw_c >= 0, else 0
 *     at each of the 8 corners that is kept, with w8 = (w_x * w_y) * w_z its trilinear weight:
 *       grad_density[row] += w8 * d_sigma;  grad_sh[row, c * B + k] += w8 * d_coef(c, k) (zero terms are not added);
 *       mask[row] = 1 - for EVERY kept corner of EVERY shaded sample, whatever its weight (svox2's sparse_grad_indexer)
 * A ray that misses the box or whose set-up is not finite writes its rgb_out (the background) and no gradient.
 * The adds are float atomics (one hardware add each, no compare-and-swap): two calls on the same input agree to rounding of
 * the sums, not bit for bit. beta_loss, sparsity_loss, background layers, randomize and last_sample_opaque are not built
 * in this call: NERF_E_INVALID naming the feature (nerf_grid_fused_backward_losses, below, has the two losses).
 *
 * nerf_grid_tv_grad: for the `count` nodes (start + i) mod X Y Z, i < count (svox2's contiguous random cells) and the columns
 * [start_dim, end_dim) of the density or the SH table, with v000 the node's value and v100, v010, v001 its +x, +y, +z
 * neighbours' (an empty or out-of-range node is 0 and receives nothing):
 *   dx = v100 - v000, dy, dz likewise;  idelta = scale / sqrt(((1e-9 + dx dx) + dy dy) + dz dz)
 *   dx *= X / 256, dy *= Y / 256, dz *= Z / 256
 *   grad[v100] += dx * idelta, grad[v010] += dy * idelta, grad[v001] += dz * idelta, grad[v000] += -((dx + dy) + dz) * idelta
 * each only if the value added is not zero, and then mask[row] = 1. ignore_edge, ignore_last_z and NDC are not built in this
 * call (nerf_grid_tv_grad_edge, below, has ignore_edge).
 *
 * nerf_grid_optim_step: elementwise over data [rows, cols] in the rows whose mask byte is set; other rows, and their rms,
 * are not touched. fp32, each operation correctly rounded, in this order:
 *   RMSProp: g2 = g * g;  rms = (rms == 0) ? g2 : g2 + beta * (rms - g2);
 *            data = max(data - (lr * g) / (sqrt(rms) + eps), minval)
 *   SGD:     data = max(data - lr * g, minval)
 * (svox2 passes minval = -1e9 for densities and colours). `data` is normally the grid's own density_data or sh_data.
 * Every operation is IEEE fp32: subnormal operands and results are kept (on a first touch a g whose square underflows to 0
 * leaves rms = 0 and steps by lr * g / eps, with eps = 0 by +-inf or NaN), -0 is a zero, and any non-zero mask byte selects
 * its row.
 * `max` is C fmaxf, as in svox2's CUDA: a NaN operand is dropped, so an element whose new value is NaN (a NaN gradient or
 * rms, inf - inf, 0 / 0) becomes minval; a NaN that reaches rms is stored there and stays. +-inf follow IEEE arithmetic. */
typedef struct nerf_grid_fused_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]                                                                */
    const float* dirs;          /* [dev] [n_rays, 3], need not be unit                                              */
    const float* rgb_gt;        /* [dev] [n_rays, 3]                                                                */
    int64_t n_rays;             /* 0: nothing is done                                                               */
    float* rgb_out;             /* [dev] [n_rays, 3]                                                                */
    float* log_transmit;        /* [dev] [n_rays] or NULL                                                           */
    float* grad_density;        /* [dev] [capacity, 1], added to                                                    */
    float* grad_sh;             /* [dev] [capacity, 3 * basis_dim], added to                                        */
    uint8_t* mask;              /* [dev] [capacity]                                                                 */
    float beta_loss;            /* must be 0 (not built) except in nerf_grid_fused_backward_losses                  */
    float sparsity_loss;        /* must be 0 (not built) except in nerf_grid_fused_backward_losses                  */
    int32_t background_nlayers; /* must be 0 (not built)                                                            */
    int32_t use_skip;           /* 1: use the skip data if nerf_grid_accelerate made it                             */
    void* stream;
} nerf_grid_fused_args;

#define NERF_GRID_TV_DENSITY 0
#define NERF_GRID_TV_SH 1
typedef struct nerf_grid_tv_args {
    size_t struct_size;
    int32_t target;             /* NERF_GRID_TV_DENSITY / NERF_GRID_TV_SH: the grid's table that is differentiated   */
    int32_t start_dim, end_dim; /* columns of that table                                                            */
    int64_t start, count;       /* nodes (start + i) mod X Y Z; 0 <= start < X Y Z, 0 <= count <= X Y Z              */
    float scale;
    int32_t ignore_edge;        /* must be 0 (not built) except in nerf_grid_tv_grad_edge: 0 or 1                   */
    int32_t ignore_last_z;      /* must be 0 (not built)                                                            */
    int32_t use_ndc;            /* must be 0 (not built)                                                            */
    float* grad;                /* [dev] shaped like the table, added to                                            */
    uint8_t* mask;              /* [dev] [capacity]                                                                 */
    void* stream;
} nerf_grid_tv_args;

#define NERF_GRID_OPTIM_RMSPROP 0
#define NERF_GRID_OPTIM_SGD 1
typedef struct nerf_grid_optim_args {
    size_t struct_size;
    float* data;                /* [dev] [rows, cols], updated in place                                             */
    float* rms;                 /* [dev] [rows, cols] running mean of g^2 (RMSProp; may be NULL for SGD)             */
    const float* grad;          /* [dev] [rows, cols]                                                               */
    const uint8_t* mask;        /* [dev] [rows]                                                                     */
    int64_t rows;
    int32_t cols;
    int32_t kind;               /* NERF_GRID_OPTIM_RMSPROP / NERF_GRID_OPTIM_SGD                                    */
    float beta, lr, eps, minval;
    void* stream;
} nerf_grid_optim_args;

int nerf_grid_fused_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_fused_args* args);
int nerf_grid_tv_grad(nerf_sparse_grid* grid, const nerf_grid_tv_args* args);
int nerf_grid_optim_step(nerf_ctx* ctx, const nerf_grid_optim_args* args);

/* Sparse voxel grid: training with the beta and sparsity losses -----------------------------------
 * What svox2's published configurations add to the step above: the two regularisers its volume_render_cuvol_fused folds into
 * the density gradient of the same march (lambda_beta, lambda_sparsity), and the edge rule its inplace_tv_color_grad always
 * runs with (ignore_edge). The capability has entries of its own: nerf_grid_fused_backward, nerf_grid_render_backward,
 * nerf_grid_tv_grad and nerf_grid_background_backward keep refusing these fields. The device code is shared; the terms are a
 * compile-time variant of the same kernels, so the entries above launch the code they launched before. All three calls are
 * stream-ordered, synchronise nothing, and ACCUMULATE as above.
 *
 * nerf_grid_fused_backward_losses is nerf_grid_fused_backward - the same struct, the same contract: rgb_out and log_transmit
 * bit-identical to nerf_grid_render_rays, background_nlayers, randomize and last_sample_opaque refused, zero rays do nothing -
 * and honours beta_loss and sparsity_loss, both finite and >= 0 (else NERF_E_INVALID naming the field); with both 0 it IS
 * nerf_grid_fused_backward (the same kernel). For a ray that is marched, fp32, each operation rounded, in this order
 * (trace_ray_cuvol_backward):
 *   T_in   = exp(log_T_final)     the forward's final log_transmit of this ray (-1e3 where it stopped, so T_in = 0); in the
 *                                 fused kernel it is the first march's own value, nothing goes through memory
 *   c_beta = beta_loss * (1 - T_in / ((1 - T_in) + 1e-3))                        only if beta_loss > 0
 *   at every shaded sample (sigma > sigma_thresh), after accum = fp32(sum_c remaining_c g_c) is formed as above:
 *     accum'  = accum + c_beta                                                    only if beta_loss > 0
 *     d_sigma = (step_size * delta_scale) * (exp(log_T after the sample) * dot - accum')
 *     d_sigma = d_sigma + sparsity_loss * ((4 sigma) / (1 + 2 (sigma sigma)))     only if sparsity_loss > 0
 * and everything else - d_coef, the corner weights, zero terms not added, the mask at every kept corner of every shaded
 * sample - is as above: grad_sh and the set of touched rows do not depend on the two weights. c_beta is the derivative of
 *   beta_loss * sum_ray [log_T + log((1 - exp(log_T)) + 1e-3)]
 * with respect to the ray's final log_T, and the last line that of sparsity_loss * sum over shaded samples of
 * log(1 + 2 sigma^2) with respect to the sample's sigma. beta_loss is applied as given: svox2 passes lambda_beta / n_rays
 * to its kernel, and so does this project's Python.
 *
 * nerf_grid_render_backward_losses is nerf_grid_render_backward (args: that call's struct, every rule of it) and takes the
 * terms in a struct of its own. T_in comes from losses->log_transmit[ray], the taped foreground render's log_transmit; it is
 * required when beta_loss > 0. The terms touch grad_density only: a NULL grad_density together with a non-zero weight is
 * NERF_E_INVALID. c_beta is no part of the tape: a background pass that continues from the tape never sees it (svox2 removes
 * it from its accum_out again). With both weights 0 it is nerf_grid_render_backward (the same kernel).
 *
 * nerf_grid_tv_grad_edge is nerf_grid_tv_grad - the same struct, the same checks, target SH refused on a half-precision
 * handle - and honours ignore_edge in {0, 1}; with 0 it IS nerf_grid_tv_grad (the same kernel). With 1
 * (tv_grad_sparse_kernel with ignore_edge = true):
 *   a cell whose own link is exactly row 0 does nothing (the reference's literal `*links_ptr == 0`, followed literally:
 *     it is what its checkpoints were trained with);
 *   v000 = the cell's own value, 0 where the cell itself is empty;
 *   a neighbour that is empty or lies outside the lattice reads v000 instead of 0: its difference is 0 and it receives nothing;
 *   so an empty cell still contributes the differences towards its kept neighbours, and a kept cell none towards empty ones;
 *   idelta, the scales X / 256, Y / 256, Z / 256, zero terms not added and the mask are as in nerf_grid_tv_grad.
 * ignore_last_z (it belongs to last_sample_opaque) and use_ndc are refused as there. */
struct nerf_grid_render_backward_args;      /* "Sparse voxel grid: gradients for autograd", below */
typedef struct nerf_grid_render_backward_losses_args {
    size_t struct_size;
    float beta_loss;            /* finite, >= 0; applied as given                                                   */
    float sparsity_loss;        /* finite, >= 0                                                                     */
    const float* log_transmit;  /* [dev] [n_rays] of the taped foreground render; required when beta_loss > 0       */
} nerf_grid_render_backward_losses_args;

int nerf_grid_fused_backward_losses(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_fused_args* args);
int nerf_grid_render_backward_losses(nerf_sparse_grid* grid, const nerf_grid_render_options* opt,
                                     const struct nerf_grid_render_backward_args* args,
                                     const nerf_grid_render_backward_losses_args* losses);
int nerf_grid_tv_grad_edge(nerf_sparse_grid* grid, const nerf_grid_tv_args* args);

/* Sparse voxel grid: gradients for autograd -------------------------------------------------------
 * The two halves of nerf_grid_fused_backward as calls of their own, with the cotangent d loss / d rgb supplied by the caller
 * between them, and the transpose of nerf_grid_sample: what a torch.autograd.Function needs to differentiate a render or a
 * sample with respect to density_data and sh_data under any loss. All three are stream-ordered, synchronise nothing and
 * return a status with nerf_last_error(). Gradients ACCUMULATE, as in the training section: the caller zeroes them.
 *
 * nerf_grid_render_rays_taped is nerf_grid_render_rays (rgb_out and log_transmit bit-identical to it, with and without skip
 * data) and also writes the tape, tape[ray, c] in fp64: the colour of channel c once more as the fp64 sum of the exact
 * products weight * max(0, raw_c) of all shaded samples plus exp(log_T) * background_brightness - the starting value of
 * `remaining_c` in the training section. 24 bytes per ray; nothing else is kept between forward and backward.
 *
 * nerf_grid_render_backward marches every ray once more over the same sample lattice under the same options (the same fp32
 * additions of t, sigma_thresh and stop rules, skip data) and adds the gradients of sum_ray,c grad_rgb[ray, c] * rgb[ray, c]
 * to grad_density and grad_sh: the statement of nerf_grid_fused_backward operation for operation - dot, the fp64 remaining
 * (started from tape[ray, c]), accum, d_sigma, d_coef, the corner weights (w_x * w_y) * w_z, zero terms not added, the
 * mask at every kept corner of every shaded sample - with g_c = grad_rgb[ray, c] instead of the MSE's. origins, dirs, the
 * options, use_skip and the grid's tables must be those of the taped render. A ray that misses the box or whose set-up is
 * not finite contributes nothing. grad_density, grad_sh and mask may each be NULL: that table's adds (the mask's stores) are
 * not issued. The adds are float atomics (one hardware add each, no compare-and-swap): two calls agree to rounding of the
 * sums, not bit for bit.
 *
 * nerf_grid_sample_backward: for every point p (cell, weights and world-to-grid transform exactly those of
 * nerf_grid_sample) and every column j (0 = density, 1.. = sh; with want_colors = 0 the density column only), at each of
 * the 8 corners whose link is kept:
 *   table[row, j] += ((w_x * grad_out[p, j]) * w_y) * w_z        (fp32, each product rounded, in this order: the
 *                                                                 reference's; a product that is zero is not added)
 * A NULL grad_density or grad_sh skips that table. There is no gradient with respect to the points. */
typedef struct nerf_grid_render_taped_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]                                                                */
    const float* dirs;          /* [dev] [n_rays, 3], need not be unit                                              */
    int64_t n_rays;             /* 0: nothing is done                                                               */
    float* rgb_out;             /* [dev] [n_rays, 3]                                                                */
    float* log_transmit;        /* [dev] [n_rays] or NULL                                                           */
    double* tape;               /* [dev] [n_rays, 3]                                                                */
    int32_t use_skip;           /* 1: use the skip data if nerf_grid_accelerate made it                             */
    void* stream;
} nerf_grid_render_taped_args;

typedef struct nerf_grid_render_backward_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]       (those of the taped render)                              */
    const float* dirs;          /* [dev] [n_rays, 3]                                                                */
    int64_t n_rays;             /* 0: nothing is done                                                               */
    const float* grad_rgb;      /* [dev] [n_rays, 3] d loss / d rgb_out, contiguous                                 */
    const double* tape;         /* [dev] [n_rays, 3] as nerf_grid_render_rays_taped wrote it                        */
    float* grad_density;        /* [dev] [capacity, 1], added to; or NULL                                           */
    float* grad_sh;             /* [dev] [capacity, 3 * basis_dim], added to; or NULL                               */
    uint8_t* mask;              /* [dev] [capacity] or NULL                                                         */
    int32_t use_skip;
    void* stream;
} nerf_grid_render_backward_args;

typedef struct nerf_grid_sample_backward_args {
    size_t struct_size;
    const float* points;        /* [dev] [n, 3] world coordinates, or grid coordinates with grid_coords              */
    int64_t n;                  /* 0: nothing is done                                                               */
    int32_t grid_coords;
    int32_t want_colors;
    const float* grad_out_density; /* [dev] [n, 1]                                                                  */
    const float* grad_out_sh;   /* [dev] [n, 3 * basis_dim]; may be NULL without want_colors or without grad_sh      */
    float* grad_density;        /* [dev] [capacity, 1], added to; or NULL                                           */
    float* grad_sh;             /* [dev] [capacity, 3 * basis_dim], added to; or NULL                               */
    void* stream;
} nerf_grid_sample_backward_args;

int nerf_grid_render_rays_taped(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_render_taped_args* args);
int nerf_grid_render_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_render_backward_args* args);
int nerf_grid_sample_backward(nerf_sparse_grid* grid, const nerf_grid_sample_backward_args* args);

/* Sparse voxel grid: resampling -------------------------------------------------------------------
 * The stages of svox2's SparseGrid.resample (coarse-to-fine training: sample the grid on another lattice, drop the nodes that
 * matter to no camera or hold no density, rebuild links). Every stage is stream-ordered and synchronises nothing; the caller
 * reads the kept-node count of nerf_grid_compact to allocate the new tables, and that is the only wait of a resample.
 * A lattice [X', Y', Z'] has at most 2^30 nodes with every side in [2, 1024]; volumes and masks are dense, C order, z fastest.
 *
 * nerf_grid_lattice_density: density[x, y, z] = the old grid's density at the point (xs[x], ys[y], zs[z]), given in the OLD
 * grid's coordinates (svox2 computes them as linspace(f - 0.5, R - f - 0.5, R') with f = 0.5 R / R' in fp32; they arrive as
 * data, nothing about them is re-derived on the device). The value is nerf_grid_sample's with grid_coords at that point, bit
 * for bit: the same clamp, cell, weights and trilinear order.
 *
 * nerf_grid_weight_render (svox2 grid_weight_render): for every pixel of `cam`, with the ray of nerf_grid_gen_rays and
 * offset / scaling of a grid of `reso`, `radius`, `center` as nerf_grid_create computes them; fp32, each operation rounded,
 * no fused multiply-adds, in this order:
 *   dn = sqrt((dx dx + dy dy) + dz dz);  o_i = offset_i + origin_i * scaling_i;  d_i = (dir_i / dn) * scaling_i
 *   delta_scale = 1 / sqrt((d_x d_x + d_y d_y) + d_z d_z);  world_step = delta_scale * step_size;  d_i = d_i * delta_scale
 *   t = 0, tmax = 2e3;  per axis with d_i != 0: t1 = (-0.5 - o_i) * (1 / d_i), t2 = ((reso_i - 0.5) - o_i) * (1 / d_i),
 *     t = max(t, min(t1, t2)), tmax = min(tmax, max(t1, t2));  a ray with not (t <= tmax), or whose set-up is not finite,
 *     returns at once
 *   log_T = 0;  while t <= tmax:
 *     p_i = clamp(o_i + t * d_i, 0, reso_i - 1);  l_i = min(int(p_i), reso_i - 2);  wb_i = p_i - l_i;  wa_i = 1 - wb_i
 *     sigma = trilinear over density at the 8 corners of cell l (z, then y, then x, as in the renderer)
 *     if sigma > 1e-8:  log_att = (-world_step) * sigma;  weight = exp(log_T) * (1 - exp(log_att));  log_T = log_T + log_att
 *       max_weight[each of the 8 corners] = max(itself, weight);  if exp(log_T) < stop_thresh: stop
 *     t = t + step_size
 * max_weight is raised, never lowered: zero it before the first camera; it must hold no negative value and no NaN (not checked:
 * the integer maximum below orders only non-negative floats). weight >= 0, so the maximum is taken as an unsigned
 * integer maximum of the float's bits (one hardware atomic, no compare-and-swap): the volume does not depend on the order in
 * which rays arrive, two calls give identical bits. last_sample_opaque is not built (NERF_E_INVALID).
 *
 * nerf_grid_threshold: mask[i] = volume[i] >= threshold (bytes 0 / 1; NaN is not kept).
 * nerf_grid_dilate: one step of the OR over the 27-neighbourhood, neighbour indices clamped at the faces (svox2 dilate);
 * `in` and `out` must not overlap.
 * nerf_grid_compact: links[node] = the number of kept nodes before it in C order if mask[node] != 0, else -1; *count = the
 * number of kept nodes. Deterministic (counts per 1024 nodes, one scan, no atomics). block_offsets is a workspace of
 * nerf_grid_compact_workspace(nodes) int32.
 * nerf_grid_gather: the tables of the new grid from `links` of nerf_grid_compact and `rows` = its count: for the kept node
 * n of row r, density_data[r] = lattice_density[n] (the value the threshold saw) and sh_data[r, :] = the old grid's SH
 * coefficients interpolated at (xs, ys, zs)[n] as nerf_grid_sample does. node_of_row is a workspace of `rows` int32. */
typedef struct nerf_grid_lattice_args {
    size_t struct_size;
    int32_t reso[3];            /* the new lattice                                                                  */
    const float* xs;            /* [dev] [reso[0]] node coordinates in the old grid's coordinates                    */
    const float* ys;            /* [dev] [reso[1]]                                                                  */
    const float* zs;            /* [dev] [reso[2]]                                                                  */
    float* density;             /* [dev] [X', Y', Z']                                                               */
    void* stream;
} nerf_grid_lattice_args;

typedef struct nerf_grid_weight_args {
    size_t struct_size;
    int32_t reso[3];
    float radius[3];            /* > 0: the geometry of the grid the volume belongs to                              */
    float center[3];
    const float* density;       /* [dev] [X', Y', Z']                                                               */
    float* max_weight;          /* [dev] [X', Y', Z'], raised                                                       */
    float step_size;            /* svox2 uses 0.5; >= 1e-3                                                          */
    float stop_thresh;          /* svox2's weight_render_stop_thresh, 0.2                                           */
    int32_t last_sample_opaque; /* must be 0 (not built)                                                            */
    void* stream;
} nerf_grid_weight_args;

typedef struct nerf_grid_compact_args {
    size_t struct_size;
    int32_t reso[3];
    const uint8_t* mask;        /* [dev] [X', Y', Z']                                                               */
    int32_t* links;             /* [dev] [X', Y', Z']                                                               */
    int32_t* block_offsets;     /* [dev] [nerf_grid_compact_workspace(X' Y' Z')] workspace                          */
    int32_t* count;             /* [dev] [1]                                                                        */
    void* stream;
} nerf_grid_compact_args;

typedef struct nerf_grid_gather_args {
    size_t struct_size;
    int32_t reso[3];
    const float* xs;            /* as in nerf_grid_lattice_args                                                     */
    const float* ys;
    const float* zs;
    const int32_t* links;       /* [dev] [X', Y', Z'] from nerf_grid_compact                                        */
    const float* lattice_density; /* [dev] [X', Y', Z'] from nerf_grid_lattice_density                              */
    int64_t rows;               /* the count of nerf_grid_compact; 0: nothing is done                               */
    int32_t* node_of_row;       /* [dev] [rows] workspace                                                           */
    float* density_data;        /* [dev] [rows, 1]                                                                  */
    float* sh_data;             /* [dev] [rows, 3 * basis_dim of `grid`]                                            */
    void* stream;
} nerf_grid_gather_args;

int nerf_grid_lattice_density(nerf_sparse_grid* grid, const nerf_grid_lattice_args* args);
int nerf_grid_weight_render(nerf_ctx* ctx, const nerf_grid_camera* cam, const nerf_grid_weight_args* args);
int nerf_grid_threshold(nerf_ctx* ctx, const float* volume, int64_t n, float threshold, uint8_t* mask, void* stream);
int nerf_grid_dilate(nerf_ctx* ctx, const int32_t* reso, const uint8_t* in, uint8_t* out, void* stream);
int64_t nerf_grid_compact_workspace(int64_t nodes);
int nerf_grid_compact(nerf_ctx* ctx, const nerf_grid_compact_args* args);
int nerf_grid_gather(nerf_sparse_grid* grid, const nerf_grid_gather_args* args);

/* Sparse voxel grid: connected components ---------------------------------------------------------
 * The connected components of a grid's occupied nodes: what the Floater Detection Ratio of svox2's
 * opt/util/advanced_metrics.py (compute_FDR) needs from scipy.ndimage.label / ndimage.sum, on the device, and the two
 * stages with which the components it calls floaters are removed from a grid. Every call except
 * nerf_grid_components_finish is stream-ordered, allocates nothing and synchronises nothing. Volumes are dense, C order,
 * z fastest; a lattice has at most 2^30 nodes with every side in [2, 1024].
 *
 * nerf_grid_components_occupancy: occupied[x, y, z] = 1 when links[x, y, z] >= 0 and, with use_density != 0,
 * density_data[links[x, y, z], 0] > threshold (an fp32 comparison; NaN is not occupied); else 0. Any negative link is empty,
 * not only -1. (compute_FDR thresholds only when `use_density_threshold and threshold > 0`: that decision is the caller's.)
 *
 * nerf_grid_components_label: two occupied nodes are neighbours when they differ by at most 1 in every coordinate and in
 * at most 1 (connectivity 6: faces), 2 (18: + edges) or 3 (26: + corners) coordinates; nothing wraps around at the faces
 * of the lattice; any other connectivity is NERF_E_INVALID. Components are numbered 1..n in increasing order of their
 * smallest flat C-order index (scipy.ndimage.label's numbering); labels[node] is the number of the node's component, 0 for a
 * node that is not occupied. status[0] = n; status[1] = the error word, 0 unless a bounded loop of the labelling hit its cap
 * or met a parent it cannot have written (a bug or memory overwritten from outside; the labels are then not to be used).
 * The labelling is a union-find whose only racing writes are integer minima, so two calls give identical bits. parent is a
 * workspace of X Y Z int32, block_offsets one of nerf_grid_components_workspace(X Y Z) int32.
 *
 * nerf_grid_components_finish: the one wait. Copies status to the host and waits for the stream: *count = status[0];
 * NERF_E_INTERNAL when the error word is set.
 *
 * nerf_grid_components_volumes: volumes[k] = the number of nodes with labels == k + 1, for k < count (zeroed first; integer
 * additions, so the result does not depend on their order). Labels outside [1, count] are ignored.
 *
 * nerf_grid_components_keep: mask[node] = 1 when links[node] >= 0 and not (labels[node] in [1, count] and
 * floater[labels[node] - 1] != 0), else 0: a kept node that is not occupied (label 0) stays.
 *
 * nerf_grid_copy_rows: the tables of a grid that keeps a subset of another grid's nodes on the same lattice. For every node
 * with new_links[node] in [0, new_rows) and old_links[node] in [0, old_rows): row new_links[node] of density / sh = row
 * old_links[node] of old_density / old_sh, copied as 32-bit words (every bit pattern survives, NaN payloads included).
 * src_row is a workspace of new_rows int32. new_rows = 0: nothing is done. old_rows is the old grid's capacity, in [0, 2^31): it
 * may exceed the nodes of the lattice (rows no link names); new_rows is at most old_rows and at most the nodes. */
#define NERF_E_INTERNAL (-5)    /* a device-side consistency check failed   */

typedef struct nerf_grid_occupancy_args {
    size_t struct_size;
    int32_t use_density;        /* 0: occupied = kept                                                               */
    float threshold;            /* not NaN                                                                          */
    uint8_t* occupied;          /* [dev] [X, Y, Z] of the grid                                                      */
    void* stream;
} nerf_grid_occupancy_args;

typedef struct nerf_grid_label_args {
    size_t struct_size;
    int32_t reso[3];
    int32_t connectivity;       /* 6, 18 or 26                                                                      */
    const uint8_t* occupied;    /* [dev] [X, Y, Z]                                                                  */
    int32_t* parent;            /* [dev] [X, Y, Z] workspace                                                        */
    int32_t* block_offsets;     /* [dev] [nerf_grid_components_workspace(X Y Z)] workspace                          */
    int32_t* labels;            /* [dev] [X, Y, Z]                                                                  */
    int32_t* status;            /* [dev] [2]: component count, error word                                           */
    void* stream;
} nerf_grid_label_args;

typedef struct nerf_grid_copy_rows_args {
    size_t struct_size;
    int32_t reso[3];
    int32_t cols;               /* columns of sh: 3 * basis_dim, >= 1                                               */
    const int32_t* old_links;   /* [dev] [X, Y, Z]                                                                  */
    const int32_t* new_links;   /* [dev] [X, Y, Z]                                                                  */
    int64_t old_rows;
    int64_t new_rows;
    const float* old_density;   /* [dev] [old_rows, 1]                                                              */
    const float* old_sh;        /* [dev] [old_rows, cols]                                                           */
    int32_t* src_row;           /* [dev] [new_rows] workspace                                                       */
    float* density;             /* [dev] [new_rows, 1]                                                              */
    float* sh;                  /* [dev] [new_rows, cols]                                                           */
    void* stream;
} nerf_grid_copy_rows_args;

int nerf_grid_components_occupancy(nerf_sparse_grid* grid, const nerf_grid_occupancy_args* args);
int64_t nerf_grid_components_workspace(int64_t nodes);
int nerf_grid_components_label(nerf_ctx* ctx, const nerf_grid_label_args* args);
int nerf_grid_components_finish(nerf_ctx* ctx, const int32_t* status, int64_t* count, void* stream);
int nerf_grid_components_volumes(nerf_ctx* ctx, const int32_t* labels, int64_t n, int64_t count, int32_t* volumes, void* stream);
int nerf_grid_components_keep(nerf_ctx* ctx, const int32_t* links, const int32_t* labels, int64_t n, const uint8_t* floater,
                              int64_t count, uint8_t* mask, void* stream);
int nerf_grid_copy_rows(nerf_ctx* ctx, const nerf_grid_copy_rows_args* args);

/* Sparse voxel grid: depth and ray lengths ----------------------------------------------------------
 * How far a ray goes before it ends: svox2's volume_render_depth (trace_ray_expected_term and trace_ray_sigma_thresh of
 * render_lerp_kernel_cuvol.cu) and the ray length of its PyTorch renderer (return_raylen). All three modes use the ray set-up
 * and the sample lattice of nerf_grid_render_rays, operation by operation: the same o, d, delta_scale, tmin (near_clip
 * applied) and tmax, the same fp32 additions of t, the same skip rule, the same stall rule. Directions need not be unit.
 * background_brightness is not read. With world_step = step_size * delta_scale (the length of a step in world units):
 *
 * NERF_GRID_DEPTH_EXPECTED: depth = 0, log_T = 0; at every sample with sigma > opt.sigma_thresh, with a and log_T as in the
 *   render:  weight = exp(log_T) (1 - exp(a));  depth += (weight * (t / step_size)) * world_step;  log_T += a;
 *   if exp(log_T) < opt.stop_thresh: log_T = -1e3, stop.  Each fp32 operation rounded, in that order. The value is the
 *   expected length along the ray in world units (not z-depth) and is NOT divided by the accumulated opacity 1 - exp(log_T):
 *   log_transmit returns log_T (bit for bit what the render returns under the same options) so that callers can normalise.
 * NERF_GRID_DEPTH_THRESHOLD: depth = (t / step_size) * world_step at the first lattice sample whose interpolated density
 *   strictly exceeds sigma_thresh, 0 if there is none. opt.sigma_thresh and opt.stop_thresh are not read. sigma_thresh < 0
 *   or NaN is NERF_E_INVALID: the skip data is only valid when an all-empty cell (sigma == 0 exactly) can never be a hit.
 * NERF_GRID_DEPTH_RAYLEN: depth = tmax - tmin, in GRID units, negative for a ray that misses the box (svox2.py
 *   _volume_render_gradcheck_lerp(return_raylen=True)). Nothing is marched; skip data is not read.
 * A ray that misses the box gives depth 0 and log_T 0. A ray whose set-up is not finite (a zero direction, a NaN or an
 * infinity in origin or direction) gives depth 0 and log_T 0, and ray length NaN. log_transmit may only be asked for in the
 * expected mode. Stream-ordered, nothing is synchronised or allocated; one lane per ray, no atomics: two calls give
 * identical bits, with and without skip data. At most 2^26 rays or pixels per call. */
#define NERF_GRID_DEPTH_EXPECTED 0
#define NERF_GRID_DEPTH_THRESHOLD 1
#define NERF_GRID_DEPTH_RAYLEN 2

typedef struct nerf_grid_depth_args {
    size_t struct_size;
    int32_t mode;               /* NERF_GRID_DEPTH_*                                                                */
    float sigma_thresh;         /* NERF_GRID_DEPTH_THRESHOLD: >= 0, not NaN; otherwise not read                     */
    const float* origins;       /* [dev] [n_rays, 3]       (nerf_grid_depth_rays only)                              */
    const float* dirs;          /* [dev] [n_rays, 3], need not be unit                                              */
    int64_t n_rays;             /* nerf_grid_depth_image: ignored, width * height rays in row-major pixel order     */
    float* depth;               /* [dev] [n_rays]                                                                   */
    float* log_transmit;        /* [dev] [n_rays] or NULL; NERF_GRID_DEPTH_EXPECTED only                            */
    int32_t use_skip;           /* 1: use the skip data if nerf_grid_accelerate made it; 0: plain march             */
    void* stream;
} nerf_grid_depth_args;

int nerf_grid_depth_rays(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_depth_args* args);
/* the rays of `cam` made inside the launch (as nerf_grid_render_image makes them): one call per frame */
int nerf_grid_depth_image(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
                          const nerf_grid_depth_args* args);

/* Sparse voxel grid: gradients of depth and log_transmit for autograd -------------------------------
 * The expected depth (NERF_GRID_DEPTH_EXPECTED) and log_T of the section above as a forward that leaves a tape and a backward
 * that takes a cotangent for each: what a torch.autograd.Function needs to differentiate depth maps, silhouettes and opacity
 * regularisers with respect to density_data under any loss. Both depend on density_data alone: sh_data is not read and has
 * no gradient. Both calls are stream-ordered, synchronise and allocate nothing and return a status with nerf_last_error().
 * Gradients ACCUMULATE, as in the sections on training and on autograd: the caller zeroes them. At most 2^26 rays per call.
 * The threshold depth is piecewise constant and the ray length does not depend on the tables: neither has a backward.
 *
 * nerf_grid_depth_rays_taped is nerf_grid_depth_rays in mode NERF_GRID_DEPTH_EXPECTED (depth and log_transmit bit-identical
 * to it, with and without skip data) and also writes the tape, tape[ray] in fp64: the ray's depth once more, as the fp64 sum
 * of the very fp32 terms  term = (weight * (t / step_size)) * world_step  that the forward adds in fp32 (0 for a ray that is
 * not marched). 8 bytes per ray; nothing else is kept between forward and backward.
 *
 * nerf_grid_depth_backward marches every ray once more over the same sample lattice under the same options (the same fp32
 * additions of t, the same sigma_thresh and stop rules, the same skip rule, the same stall rule) and adds to grad_density
 * the gradient of  sum_ray grad_depth[ray] * depth[ray] + grad_log_transmit[ray] * log_transmit[ray].  origins, dirs, the
 * options, use_skip and the grid's tables must be those of the taped forward. Per ray: g_d = grad_depth[ray] and
 * g_T = grad_log_transmit[ray], each 0 where the pointer is NULL; step_ds = step_size * delta_scale (= world_step);
 * neg_step = -step_size; remaining = tape[ray] (fp64; 0 without a tape); log_T = 0. At every sample with
 * sigma > opt.sigma_thresh, in march order, fp32 with each operation rounded, in this order:
 *   a      = (neg_step * sigma) * delta_scale
 *   weight = exp(log_T) * (1 - exp(a))
 *   tau    = t / step_size
 *   term   = (weight * tau) * world_step                       (the forward's term, bit for bit)
 *   remaining = remaining - (double)term                       (fp64: what the later samples still add to the depth)
 *   log_T  = log_T + a
 *   lead   = (exp(log_T) * tau) * world_step
 *   d_sigma = step_ds * (g_d * (lead - (float)remaining)) - g_T * step_ds
 *   at each of the 8 corners (x, y, z bits) whose link is kept:  v = ((w_x * w_y) * w_z) * d_sigma;
 *     grad_density[row] += v  unless v == 0 (a zero term is not added)
 *   if exp(log_T) < opt.stop_thresh: stop (after the adds of this sample)
 * This is  d depth / d sigma_i = step_ds (T_{i+1} tau_i world_step - sum_{j > i} term_j)  and  d log_T / d sigma_i = -step_ds.
 * A ray that stops at stop_thresh returned the constant log_T = -1e3: for such a ray g_T is taken as 0 at every sample (the
 * call finds out whether a ray with g_T != 0 stops by marching it once without adds before the march that adds), and g_d
 * contributes at the samples up to and including the stopping one, with log_T as it stood before the reset. A ray that
 * misses the box or whose set-up is not finite contributes nothing, whatever its cotangents hold. n_rays = 0 does nothing.
 * grad_depth and grad_log_transmit may each be NULL, not both (NERF_E_INVALID); tape may be NULL if and only if grad_depth
 * is. The adds are float atomics (one hardware add each, no compare-and-swap): two calls agree to rounding of the sums,
 * not bit for bit. */
typedef struct nerf_grid_depth_taped_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]                                                                */
    const float* dirs;          /* [dev] [n_rays, 3], need not be unit                                              */
    int64_t n_rays;             /* 0: nothing is done                                                               */
    float* depth;               /* [dev] [n_rays]                                                                   */
    float* log_transmit;        /* [dev] [n_rays] or NULL                                                           */
    double* tape;               /* [dev] [n_rays]                                                                   */
    int32_t use_skip;           /* 1: use the skip data if nerf_grid_accelerate made it                             */
    void* stream;
} nerf_grid_depth_taped_args;

typedef struct nerf_grid_depth_backward_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]       (those of the taped forward)                             */
    const float* dirs;          /* [dev] [n_rays, 3]                                                                */
    int64_t n_rays;             /* 0: nothing is done                                                               */
    const float* grad_depth;    /* [dev] [n_rays] d loss / d depth, or NULL                                         */
    const float* grad_log_transmit; /* [dev] [n_rays] d loss / d log_transmit, or NULL                              */
    const double* tape;         /* [dev] [n_rays] as nerf_grid_depth_rays_taped wrote it; NULL iff grad_depth is    */
    float* grad_density;        /* [dev] [capacity, 1], added to                                                    */
    int32_t use_skip;
    void* stream;
} nerf_grid_depth_backward_args;

int nerf_grid_depth_rays_taped(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_depth_taped_args* args);
int nerf_grid_depth_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_depth_backward_args* args);

/* Sparse voxel grid: floater views ------------------------------------------------------------------
 * The labelled nodes of the connected components (section "connected components") projected into a camera: what svox2's
 * opt/util/floater_visualization.py computes in Python loops on the host. Both calls scan the label tensor, one thread per
 * node, and take the node's entry in a per-label table built by the caller: table[label] for 1 <= label <= n_labels, and 0
 * (ignore) for label 0, a label outside that range or an entry of 0. Both are stream-ordered, allocate and synchronise
 * nothing and return a status with nerf_last_error(). A camera with ndc_coeffs is refused (NERF_E_INVALID): both calls project
 * world points through a pinhole, which an NDC view is not. At most 2^26 pixels.
 *
 * The projection of node (i, j, k), fp32, every operation rounded separately, no fused multiply-add, per axis a:
 *   p_a = ((idx_a / reso_a) * 2 - 1) * radius_a + center_a
 * This is the reference's formula and NOT grid2world: it has no + 0.5, so it is the voxel's lower corner, half a voxel from
 * the node the renderer samples. It is kept, so that the images are the reference's.
 *   q_r = ((w2c[r][0] p_0 + w2c[r][1] p_1) + w2c[r][2] p_2) + w2c[r][3]      r = 0, 1, 2;  w2c row-major [3, 4]
 *   x = (q_0 / q_2) * fx + cx,  y = (q_1 / q_2) * fy + cy                    fx, fy, cx, cy: the camera's, rounded to fp32
 * The node is VALID iff q_2 > 0, 0 <= x < width and 0 <= y < height (a NaN fails); (xi, yi) is the truncation of (x, y).
 * The camera's c2w is checked and not read: the caller passes w2c, the inverse of the 4 x 4 c2w rounded to fp32.
 *
 * nerf_grid_floater_heatmap (project_floaters_to_view). For every node with a non-zero table entry:
 *   rho = density_data[link] if 0 <= link < capacity, else 0; with min_density > 0 the node is dropped unless
 *     rho >= min_density                                                      counters[0] += 1 for every node kept ("dense")
 *   it must be valid and inside the heatmap: xi < out_width, yi < out_height  counters[1] += 1 ("in view")
 *   with filter_occluded, d = depth[yi * width + xi] on the camera's [height, width] map; the node is visible iff
 *     q_2 < d + 0.05 or d < 0.01. The reference compares the camera-space z with a length along the ray; that is kept.
 *                                                                             counters[2] += 1 ("visible")
 *   counts[yi * out_width + xi] += 1
 * Then heatmap = the maximum of counts over the 3 x 3 neighbours that lie inside the image (cv2.dilate with its default
 * border), as float. The reference dilates only if some count is non-zero; the maximum over an all-zero image is that image,
 * so nothing has to be decided and nothing goes to the host. counts, counters and counter_slots are zeroed by the call;
 * counter_slots is where the wavefronts add their sums, spread over 256 cache lines, before the second kernel adds them up
 * into counters.
 *
 * nerf_grid_component_view (create_multi_object_voxel_overlay's far-to-near painter with its depth test, without the random
 * subsampling to max_points_per_object that the reference has for speed only). The table holds the slot >= 1 to draw a label
 * with. Every valid node with a slot covers the 21 pixels (xi + dx, yi + dy), dx^2 + dy^2 <= 5, that lie inside the camera's
 * image: the disc is fixed here and not read from OpenCV's circle raster. slots[pixel] is the slot of the covering node
 * with the smallest q_2, among equal q_2 the smallest slot, and 0 where no node covers the pixel. keys is a workspace of one
 * uint64 per pixel, set to all ones by the call and lowered with (bits(q_2) << 32) | slot: q_2 > 0, so the bit pattern
 * orders as the float does.
 *
 * Every atomic is an integer one (add on int32, min on uint64), so every result is deterministic: two calls give identical
 * bits. */
#define NERF_GRID_FLOATER_COUNTER_INTS 8192

typedef struct nerf_grid_floater_heatmap_args {
    size_t struct_size;
    const int32_t* labels;      /* [dev] [X, Y, Z] of the grid                                                      */
    const int32_t* table;       /* [dev] [n_labels + 1]: non-zero = a floater                                        */
    int64_t n_labels;
    float radius[3];            /* of the grid (positive, finite)                                                   */
    float center[3];
    float w2c[12];              /* [3, 4] row-major                                                                 */
    float min_density;          /* <= 0: no density filter                                                          */
    int32_t filter_occluded;
    const float* depth;         /* [dev] [height, width] of the camera; may be NULL without filter_occluded         */
    int32_t out_width, out_height; /* the heatmap's size (render_size), the camera's by default                      */
    int32_t* counts;            /* [dev] [out_height, out_width] workspace: the counts before the dilation           */
    int32_t* counters;          /* [dev] [3]: dense, in view, visible                                                */
    int32_t* counter_slots;     /* [dev] [NERF_GRID_FLOATER_COUNTER_INTS] workspace                                  */
    float* heatmap;             /* [dev] [out_height, out_width]                                                    */
    void* stream;
} nerf_grid_floater_heatmap_args;

typedef struct nerf_grid_component_view_args {
    size_t struct_size;
    const int32_t* labels;      /* [dev] [X, Y, Z] of the grid                                                      */
    const int32_t* table;       /* [dev] [n_labels + 1]: the slot >= 1 of a label, 0 = not drawn                     */
    int64_t n_labels;
    float radius[3];
    float center[3];
    float w2c[12];
    uint64_t* keys;             /* [dev] [height, width] workspace                                                  */
    int32_t* slots;             /* [dev] [height, width]                                                            */
    void* stream;
} nerf_grid_component_view_args;

int nerf_grid_floater_heatmap(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_floater_heatmap_args* args);
int nerf_grid_component_view(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_component_view_args* args);

/* Sparse voxel grid: half-precision colours ---------------------------------------------------------
 * An inference-side grid whose SH table lives on the device in fp16, as a Plenoxels checkpoint stores it (svox2's
 * SparseGrid.save writes sh_data.astype(float16)). Density, links and skip data are those of section "Sparse voxel grid".
 *
 * The packed table is uint16 [capacity, nerf_grid_half_row_halfs(basis_dim)], IEEE binary16 bit patterns. One row:
 *   channel-major like sh_data; channel c starts at slot c * S with S = 10 / 4 / 1 at basis_dim 9 / 4 / 1 (basis_dim rounded
 *   up to even, so that coefficients (2 j, 2 j + 1) of a channel share an aligned 32-bit word), coefficient k of channel c is
 *   slot c * S + k; every other slot is zero. The row has 32 / 16 / 4 halfs = 64 / 32 / 8 bytes (fp32: 108 / 48 / 12), a
 *   power of two, so a row never straddles a 64-byte line. The table must be 4-byte aligned.
 * Only nerf_grid_pack_half, nerf_grid_unpack_half and the render / sample kernels know this layout; everything else goes
 * through them.
 *
 * nerf_grid_pack_half converts fp32 rows [rows, 3 * basis_dim] into rows [row0, row0 + rows) of the packed table - row0 lets a
 * loader pack in chunks and never hold a whole fp32 table. A coefficient x becomes half(clamp(x, -65504, 65504)) rounded to
 * nearest even: one that would overflow becomes the largest half and not an infinity (which would turn a sample of weight
 * zero into NaN); NaN stays NaN; signed zeros and subnormals convert as IEEE 754 does. `clamped` [dev] (or NULL) is
 * INCREMENTED by the number of entries with |x| > 65504; the caller zeroes it. nerf_grid_unpack_half is the exact widening
 * of rows [0, rows) back to fp32 [rows, 3 * basis_dim]. Both are stream-ordered and synchronise nothing.
 *
 * nerf_grid_create_half is nerf_grid_create with the packed table in place of sh_data: the same link check (it synchronises
 * `stream`), the same borrowed-pointer rules, the same opaque handle, destroyed by nerf_grid_destroy. On such a handle
 *   - nerf_grid_render_rays, nerf_grid_render_image (also with `counters`) and nerf_grid_sample read the halves. A half is
 *     widened to fp32 when it is loaded and everything after that is the fp32 arithmetic of section "Sparse voxel grid" in
 *     the same order and association, so the results are, bit for bit, those of a nerf_grid_create handle on the table of
 *     nerf_grid_unpack_half. For a grid that came from a checkpoint that is a lossless render.
 *   - every entry point that reads links and density only works unchanged: accelerate / drop_skip / has_skip, depth rays and
 *     image in all modes, depth taped / backward, lattice density, components occupancy, floater heatmap, component view.
 *   - every entry point that reads or writes an fp32 SH table through the handle returns NERF_E_INVALID and names the
 *     half-precision grid, before any launch: nerf_grid_fused_backward, nerf_grid_render_rays_taped,
 *     nerf_grid_render_backward, nerf_grid_sample_backward, nerf_grid_tv_grad with NERF_GRID_TV_SH, nerf_grid_gather.
 * lanes chooses the lane mapping of the render kernel; the results do not depend on it.
 *   NERF_GRID_HALF_LANES_SINGLE  one coefficient per lane, the mapping of the fp32 kernel: 2 / 4 / 16 rays per wavefront
 *   NERF_GRID_HALF_LANES_PAIR    two coefficients per lane from one 32-bit load: 4 / 8 rays per wavefront at basis_dim 9 / 4
 *                                (basis_dim 1 has no pairs: SINGLE)
 *   NERF_GRID_HALF_LANES_DEFAULT the faster of the two as measured on the MI355X (profiles/grid_half_ab.md) */
#define NERF_GRID_HALF_LANES_DEFAULT 0
#define NERF_GRID_HALF_LANES_SINGLE 1
#define NERF_GRID_HALF_LANES_PAIR 2

typedef struct nerf_grid_half_desc {
    size_t struct_size;         /* sizeof(nerf_grid_half_desc), checked                                             */
    int32_t reso[3];            /* nodes per axis, each in [2, 1024]                                                */
    int32_t basis_dim;          /* 1, 4 or 9                                                                        */
    float radius[3];            /* > 0                                                                              */
    float center[3];
    int64_t capacity;           /* rows of density_data / sh_half, >= 0                                             */
    const int32_t* links;       /* [dev] [X, Y, Z]                                                                  */
    const float* density_data;  /* [dev] [capacity, 1]          (may be NULL when capacity == 0)                    */
    const uint16_t* sh_half;    /* [dev] [capacity, nerf_grid_half_row_halfs(basis_dim)], as nerf_grid_pack_half writes it */
    int32_t lanes;              /* NERF_GRID_HALF_LANES_*                                                           */
    void* stream;
} nerf_grid_half_desc;

typedef struct nerf_grid_pack_half_args {
    size_t struct_size;
    int32_t basis_dim;          /* 1, 4 or 9                                                                        */
    int64_t capacity;           /* rows of the packed table                                                         */
    int64_t row0, rows;         /* rows [row0, row0 + rows) of it are written; 0 <= row0, 0 <= rows, row0 + rows <= capacity */
    const float* sh_data;       /* [dev] [rows, 3 * basis_dim]                                                      */
    uint16_t* sh_half;          /* [dev] [capacity, nerf_grid_half_row_halfs(basis_dim)]                            */
    unsigned long long* clamped; /* [dev] [1] or NULL: += entries with |x| > 65504                                  */
    void* stream;
} nerf_grid_pack_half_args;

/* halfs in one packed row: 32 / 16 / 4; NERF_E_INVALID (negative) for a basis_dim other than 9 / 4 / 1. Needs no device. */
int nerf_grid_half_row_halfs(int32_t basis_dim);
int nerf_grid_pack_half(nerf_ctx* ctx, const nerf_grid_pack_half_args* args);
int nerf_grid_unpack_half(nerf_ctx* ctx, const uint16_t* sh_half, int64_t rows, int32_t basis_dim, float* sh_data, void* stream);
int nerf_grid_create_half(nerf_ctx* ctx, const nerf_grid_half_desc* desc, nerf_sparse_grid** out);

/* Sparse voxel grid: palette-quantised colours ------------------------------------------------------
 * An inference-side grid whose colours are palette indices: for each SH basis function k the RGB triple of coefficients
 * (sh[:, k], sh[:, B + k], sh[:, 2 B + k]) of all nodes is quantised to one of 2^bits fp16 colours, and a node stores a uint16
 * index per function - PlenOctree's octree/compression.py on this project's grid. The first `retain` functions may stay as
 * fp16 triples. Density, links and skip data are those of section "Sparse voxel grid".
 *
 * The quantiser. The reference calls a C extension of svox for this step whose source is not available, so the algorithm is
 * defined here, and pinned by a numpy oracle kept with the tests (tests/grid_palette_oracle.py).
 * Balanced median cut of order `bits` over colours [m, 3] fp32, 1 <= bits <= 16:
 *   boxes      level 0 is one box holding all m members in row order. At each of `bits` levels a box j with n members
 *              becomes box 2 j with its first n - n / 2 members and box 2 j + 1 with the remaining n / 2 (integer division),
 *              after the reordering below: sizes and offsets are a pure function of (m, level, j).
 *   axis       a box with n >= 2 is split on the axis with the largest max - min (both exact, the difference rounded to fp32);
 *              ties go to the lowest axis. A box with n < 2 is not reordered.
 *   reordering a stable sort of the box's members by the fp32 value on that axis, in the order of the sign-flipped bit
 *              pattern: -0.0 sorts before +0.0, equal keys keep their current order.
 *   palette    entry j < 2^bits is the mean of final box j: summed in fp64 from -0.0 (the identity of addition, so that a box
 *              of -0.0 members keeps its sign), divided, rounded to fp32 and then to fp16 (to nearest even, clamped to
 *              +-65504): with at most one member a box the entry is half(x), bit for bit. An empty box gives (0, 0, 0). The
 *              order of the fp64 sum is the kernel's own
 *              (fixed: the same bits on every run); it may differ from another implementation's in the last bit of the sum.
 *   index      ids[i] is the final box of member i.
 * Non-finite inputs are counted on the device and refused: *nonfinite receives the number of rows with a NaN or an infinity,
 * and if it is not zero nothing is sorted, ids and palette are not written and the call returns NERF_E_INVALID. That count
 * is the only value that comes back to the host; the call synchronises `stream` for it. The sort is hipCUB's stable
 * DeviceRadixSort of (box << 32 | key, member), one per level; everything else is kernels of this library.
 * nerf_grid_median_cut_workspace(m, bits) is the size in bytes of the workspace [dev] the call needs (256-byte aligned):
 * about 32 m. It needs no device; negative (NERF_E_INVALID) for m outside [0, 2^31) or bits outside [1, 16].
 *
 * Layouts of a palette grid, Q = basis_dim - retain quantised functions, P = 2^bits:
 *   quant_map      uint16 [capacity, Q]     node-major, rows not padded (18 / 8 / 2 bytes at Q = 9 / 4 / 1): the lanes that
 *                                           walk a ray read all Q indices of one node, so these lie together. (The file's
 *                                           quant_map is the transpose, [Q, capacity], compression.py's.)
 *   quant_colors   half   [Q, P, 3]         as in the file
 *   data_retained  half   [capacity, retain, 3]   (the file's is [retain, capacity, 3])
 * nerf_grid_create_palette is nerf_grid_create with these tables in place of sh_data: the same link check, and the check that
 * every index is < 2^bits (both on the device; it synchronises `stream`), the same borrowed-pointer rules, the same opaque
 * handle, destroyed by nerf_grid_destroy. On such a handle
 *   - nerf_grid_render_rays, nerf_grid_render_image (also with `counters`) and nerf_grid_sample read a coefficient (channel c,
 *     function k) as half k < retain ? data_retained[node, k, c] : quant_colors[k - retain, quant_map[node, k - retain], c],
 *     widened to fp32 when it is loaded; everything after that is the fp32 arithmetic of section "Sparse voxel grid" in the
 *     same order and association, so the results are, bit for bit, those of a nerf_grid_create handle on the dequantised
 *     table. Skip data changes nothing, as there.
 *   - what reads links and density only and is not training works unchanged: accelerate / drop_skip / has_skip, depth rays
 *     and image in all modes, components occupancy, floater heatmap, component view.
 *   - every training, autograd, resampling and TV entry point returns NERF_E_INVALID and names the palette grid, before any
 *     launch: nerf_grid_fused_backward(_losses), nerf_grid_render_rays_taped, nerf_grid_render_backward(_losses),
 *     nerf_grid_sample_backward, nerf_grid_tv_grad(_edge), nerf_grid_tv_value(_backward), nerf_grid_sparsity_rays / _backward,
 *     nerf_grid_depth_rays_taped, nerf_grid_depth_backward, nerf_grid_lattice_density, nerf_grid_gather; and
 *     nerf_grid_set_background with a desc. */
typedef struct nerf_grid_median_cut_args {
    size_t struct_size;         /* sizeof(nerf_grid_median_cut_args), checked                                       */
    int64_t m;                  /* colours, in [0, 2^31)                                                            */
    int32_t bits;               /* in [1, 16]                                                                       */
    const float* colors;        /* [dev] [m, 3]                 (may be NULL when m == 0)                           */
    uint16_t* ids;              /* [dev] [m]                    (may be NULL when m == 0)                           */
    uint16_t* palette;          /* [dev] [2^bits, 3] binary16 bit patterns                                          */
    void* workspace;            /* [dev] workspace_bytes >= nerf_grid_median_cut_workspace(m, bits), 256-byte aligned */
    int64_t workspace_bytes;
    int64_t* nonfinite;         /* [host] out: rows with a non-finite component                                     */
    void* stream;
} nerf_grid_median_cut_args;

typedef struct nerf_grid_palette_desc {
    size_t struct_size;         /* sizeof(nerf_grid_palette_desc), checked                                          */
    int32_t reso[3];            /* nodes per axis, each in [2, 1024]                                                */
    int32_t basis_dim;          /* 1, 4 or 9                                                                        */
    float radius[3];            /* > 0                                                                              */
    float center[3];
    int64_t capacity;           /* rows of density_data / quant_map / data_retained, >= 0                           */
    int32_t bits;               /* in [1, 16]: 2^bits palette entries per function                                  */
    int32_t retain;             /* in [0, basis_dim]: functions kept as fp16 triples                                */
    const int32_t* links;       /* [dev] [X, Y, Z]                                                                  */
    const float* density_data;  /* [dev] [capacity, 1]          (may be NULL when capacity == 0)                    */
    const uint16_t* quant_map;      /* [dev] [capacity, basis_dim - retain]   (may be NULL when that is empty)      */
    const uint16_t* quant_colors;   /* [dev] [basis_dim - retain, 2^bits, 3]  (may be NULL when retain == basis_dim) */
    const uint16_t* data_retained;  /* [dev] [capacity, retain, 3]            (may be NULL when that is empty)      */
    void* stream;
} nerf_grid_palette_desc;

int64_t nerf_grid_median_cut_workspace(int64_t m, int32_t bits);
int nerf_grid_quantize_median_cut(nerf_ctx* ctx, const nerf_grid_median_cut_args* args);
int nerf_grid_create_palette(nerf_ctx* ctx, const nerf_grid_palette_desc* desc, nerf_sparse_grid** out);

/* Sparse voxel grid: background layers --------------------------------------------------------------
 * svox2's multi-sphere-image background (background_nlayers > 0), forward side: L = nlayers concentric spheres around the
 * grid's centre, radius 1 (the unit sphere of the normalised box) outwards to infinity, each an equirectangular image of
 * 2R x R texels (R = reso) holding (r, g, b, sigma).
 *   links [dev] int32 [2R, R], C order: >= 0 = row of `data`; a negative link, or one >= capacity, reads as zeros.
 *   data  [dev] float [capacity, L, 4]: channels 0..2 colour, 3 sigma; 16-byte aligned.
 * Both are BORROWED under the rules of section "Sparse voxel grid". nerf_grid_set_background attaches them to a grid of
 * nerf_grid_create (a half-precision handle is NERF_E_INVALID), checks every link against capacity on the device and
 * synchronises `stream`, as nerf_grid_create does; desc == NULL detaches. nerf_grid_has_background: 1 / 0.
 *
 * The reference states the background twice and the statements differ: its PyTorch renderer samples between consecutive
 * sphere hits and attenuates by world distance, its CUDA kernel (render_background_forward) samples ON the spheres and
 * attenuates by the difference of inverse radii. Checkpoints are trained and rendered with the CUDA kernel, so that one is
 * followed. Everything below is fp32 with every operation rounded (no fused multiply-add) unless it says fp64;
 * dot(a, b) = (a_x b_x + a_y b_y) + a_z b_z, |a| = sqrt(dot(a, a)), lerp(a, b, w) = a + w (b - a).
 *
 * The pass runs AFTER the foreground: nerf_grid_background_rays / _image take rgb [n, 3] and log_transmit [n] as the
 * foreground left them (render with background_brightness = 0 and log_transmit requested; its "+ exp(log_T) * 0" leaves the
 * colour unchanged bit for bit) and update both in place, on the same stream. Per ray, with o, d (grid-coordinate origin,
 * unit grid direction), delta_scale and the finiteness rule of the foreground's set-up, and log_T = log_transmit[ray]:
 *   if log_T < -25: the ray is left alone - nothing is read further, nothing is written, no brightness term.
 *   if the set-up is not finite (the foreground's miss rule): rgb_c += exp(log_T) * background_brightness, log_transmit
 *     is not written; no layers.
 *   Set-up, per axis a:  s_a = 2 / reso_a;  O_a = ((o_a + 0.5) * s_a) - 1;  D_a = d_a * s_a;  then
 *     inorm = 1 / |D|;  D_a = D_a * inorm;  world_step = delta_scale * inorm   (no step_size factor);
 *     q2a = 2 * dot(D, D);  qb = 2 * dot(O, D);  f = qb * qb - (2 * q2a) * dot(O, O);
 *     C = O x D (C_x = O_y * D_z - O_z * D_y, cyclic);  inner = max(|C| + 1e-3, 1);  invr_last = 1 / inner.
 *   Steps: n = (int)((float)L / step_size) + 2. For i = 0 .. n - 1:
 *     r = (float)((double)n / ((double)(n - i) - 0.5))                                       (fp64, rounded once)
 *     skip the step if r < inner;  det = f + ((2 * q2a) * r) * r;  skip the step if det < 0
 *     t = (-qb + sqrt(det)) / q2a           (the far hit; its sign is NOT tested, as in the reference: a ray that starts
 *                                            outside a sphere and points away from it is sampled behind its origin)
 *     P_a = O_a + t * D_a;  invr = 1 / |P|;  u_a = P_a * invr;  lat = asinf(u_y);  lon = atan2f(u_x, u_z)
 *     x = (float)(2R * (0.5 + ((double)lon * 0.5) * (1 / pi)));  y = (float)(R * (0.5 - (double)lat * (1 / pi)))   (fp64,
 *                                            1 / pi = 0.318309886183790671538, each rounded to fp32 once)
 *     z = fminf(fmaxf(((1 - invr) * L) - 0.5, 0), L - 1)
 *     l = (int)(x, y, z) (truncation; a NaN gives 0), each clamped to [0, (2R - 1, R - 1, L - 2)];  w = (x, y, z) - l
 *     nx = l_x + 1, or 0 at l_x = 2R - 1;  ny = l_y + 1, or 0 at l_y = R - 1   (both axes wrap)
 *     texel (X, Y) has link links[X * R + Y]; its value for channel c is
 *       lerp(data[(link * L + l_z) * 4 + c], data[(link * L + l_z + 1) * 4 + c], w_z), or 0 without a row   (z first)
 *     v_c = lerp(lerp(texel(l_x, l_y), texel(l_x, ny), w_y), lerp(texel(nx, l_y), texel(nx, ny), w_y), w_x)   (y, then x)
 *     if v_3 > 0 (sigma):  p = ((invr_last - invr) * world_step) * v_3;  weight = exp(log_T) * (1 - exp(-p));
 *       log_T = log_T - p;  out_c = out_c + weight * max(0, (v_c * 0.28209479177387814) + 0.5)  for c = 0..2;
 *       if exp(log_T) < stop_thresh: leave the loop (this step's invr_last is no longer needed)
 *     invr_last = invr                      (on every step that was not skipped, also where sigma <= 0)
 *   rgb_c = rgb_c + (out_c + exp(log_T) * background_brightness);  log_transmit[ray] = log_T.
 * sigma_thresh and near_clip are not read. Termination is unconditional: n <= L / 1e-3 + 2 with L <= 1024 and
 * step_size >= 1e-3. One lane per ray, no atomics: two calls on the same input give identical bits. The image form makes
 * the rays of `cam` inside the launch as nerf_grid_render_image does. At most 2^26 rays or pixels per call; n_rays = 0 does
 * nothing. Stream-ordered, nothing is synchronised or allocated.
 *
 * Thinning (svox2 sparsify_background), in two calls with one host read of *count between them:
 * nerf_grid_background_sparsify_plan: mask[X, Y, z] = texel (X, Y) has a row and data[link, z, 3] >= sigma_thresh (a NaN is
 *   not), dilated `dilate` times over the [2R, R, L] volume by the 27-neighbourhood clamped at the faces (svox2's dilate: no
 *   wrap); a texel is kept iff it has a row and any of its L mask bytes is set; new_links[2R, R] = the rank of a kept texel
 *   among the kept ones in C order, else -1; *count [dev] = the kept texels. (svox2 pairs the i-th texel that has a row with
 *   row i; here the texel's own link is followed, which is the same wherever svox2's pairing is valid.)
 * nerf_grid_background_gather: new_data[new_links[t]] = data[links[t]] for every kept texel t, rows of [L, 4].
 * The caller then installs new_links / new_data with nerf_grid_set_background. Deterministic; no atomics. */
typedef struct nerf_grid_background_desc {
    size_t struct_size;
    int32_t nlayers;            /* L in [2, 1024]                                                                   */
    int32_t reso;               /* R in [2, 1024]: 2R x R texels per layer                                          */
    int64_t capacity;           /* rows of data, in [0, 2^31)                                                       */
    const int32_t* links;       /* [dev] [2R, R]                                                                    */
    const float* data;          /* [dev] [capacity, L, 4], 16-byte aligned (may be NULL when capacity == 0)         */
    void* stream;
} nerf_grid_background_desc;

typedef struct nerf_grid_background_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]       (nerf_grid_background_rays only)                         */
    const float* dirs;          /* [dev] [n_rays, 3], need not be unit                                              */
    int64_t n_rays;             /* nerf_grid_background_image: ignored, width * height rays in row-major order; an NDC
                                   camera (ndc_coeffs > 0) is refused there: svox2 never combines the two          */
    float* rgb;                 /* [dev] [n_rays, 3] in / out                                                       */
    float* log_transmit;        /* [dev] [n_rays] in / out                                                          */
    void* stream;
} nerf_grid_background_args;

typedef struct nerf_grid_background_sparsify_args {
    size_t struct_size;
    int32_t nlayers, reso;      /* as in nerf_grid_background_desc                                                  */
    int64_t capacity;
    const int32_t* links;       /* [dev] [2R, R]                                                                    */
    const float* data;          /* [dev] [capacity, L, 4]                                                           */
    float sigma_thresh;         /* not NaN                                                                          */
    int32_t dilate;             /* >= 0                                                                             */
    uint8_t* mask;              /* [dev] [2, 2R, R, L] workspace (the volume and its dilation, alternating)         */
    uint8_t* keep;              /* [dev] [2R, R] workspace                                                          */
    int32_t* block_offsets;     /* [dev] [nerf_grid_compact_workspace(2 R R)] workspace                             */
    int32_t* new_links;         /* [dev] [2R, R] out                                                                */
    int32_t* count;             /* [dev] [1] out                                                                    */
    void* stream;
} nerf_grid_background_sparsify_args;

typedef struct nerf_grid_background_gather_args {
    size_t struct_size;
    int32_t nlayers, reso;
    int64_t capacity;           /* rows of data                                                                     */
    const int32_t* links;       /* [dev] [2R, R]: the old links                                                     */
    const float* data;          /* [dev] [capacity, L, 4]                                                           */
    const int32_t* new_links;   /* [dev] [2R, R] of nerf_grid_background_sparsify_plan                              */
    int64_t new_capacity;       /* *count of the plan                                                               */
    float* new_data;            /* [dev] [new_capacity, L, 4], not overlapping data                                 */
    void* stream;
} nerf_grid_background_gather_args;

int nerf_grid_set_background(nerf_sparse_grid* grid, const nerf_grid_background_desc* desc);
int nerf_grid_has_background(const nerf_sparse_grid* grid);
int nerf_grid_background_rays(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_background_args* args);
int nerf_grid_background_image(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
                               const nerf_grid_background_args* args);
int nerf_grid_background_sparsify_plan(nerf_ctx* ctx, const nerf_grid_background_sparsify_args* args);
int nerf_grid_background_gather(nerf_ctx* ctx, const nerf_grid_background_gather_args* args);

/* Sparse voxel grid: background layers, training ------------------------------------------------------
 * What svox2's optimisation loop does to the background: the background pass of volume_render_fused with a tape,
 * render_background_backward, inplace_tv_background_grad (msi_tv_grad_sparse_kernel) and optim_background_step. All four are
 * stream-ordered and synchronise nothing. Gradients ACCUMULATE: the caller zeroes grad_background [capacity, L, 4] and
 * mask_background [capacity, L] (bytes) when a new step begins. fp32, every operation rounded (no fused multiply-add),
 * unless fp64 is said. Row indices are 64-bit. The march - set-up, steps, cell, fetch, p, weight, log_T, the skip, sigma > 0
 * and stop rules - is that of section "Sparse voxel grid: background layers", the same device code.
 *
 * nerf_grid_background_rays_taped is nerf_grid_background_rays: rgb (in / out) and the new log_transmit are bit-identical to
 * that call's. It reads the foreground's log_transmit and writes the new one to log_transmit_out, so that the backward still
 * has the incoming value (the two may not be the same array). `tape` [n, 3] fp64 comes from nerf_grid_render_rays_taped of the
 * foreground, rendered with background_brightness = 0. Per ray:
 *   tape_background_c = the fp64 sum of the exact products weight * max(0, col_c) over all shaded steps, plus
 *                       (double)exp(log_T) * (double)background_brightness, with col_c = (v_c * 0.28209479177387814) + 0.5:
 *                       the background's colour without the rounding of its fp32 sum
 *   tape_c = tape_c + tape_background_c
 *   a ray left alone (log_T < -25): tape_background_c = 0, tape and rgb untouched, log_transmit_out = log_T
 *   a ray whose set-up is not finite: tape_background_c = (double)exp(log_T) * (double)background_brightness, added to tape_c
 *     too; log_transmit_out = log_T
 * The combined tape makes the foreground's nerf_grid_render_backward complete without any change to it: started from it,
 * `remaining` after a ray's last foreground sample is the background's colour (svox2's accum carried from the foreground
 * kernel into the background one).
 *
 * nerf_grid_background_backward marches every ray once more from the foreground's log_transmit, with g_c = grad_rgb[ray, c]
 * and remaining_c = tape_background[ray, c] (fp64, for the reason given in the training section). At every shaded step
 * (v_3 > 0), with p, weight, log_T as in the forward:
 *   dot = (max(0, col_0) g_0 + max(0, col_1) g_1) + max(0, col_2) g_2
 *   remaining_c -= weight * max(0, col_c)   (fp64, exact products);   accum = fp32(sum_c remaining_c g_c)   (c = 0, 1, 2)
 *   d_3 = ((invr_last - invr) * world_step) * (exp(log_T after the step) * dot - accum)                      (sigma)
 *   d_c = (0.28209479177387814 * weight) * g_c  where col_c > 0 (strict, as the reference), else 0           (colours)
 *   for each of the 4 texels (X, Y) in {l_x, nx} x {l_y, ny} that has a row, and every channel c = 0..3:
 *     xo = (1 - w_x) * d_c at X = l_x, w_x * d_c at X = nx;   val = (1 - w_y) * xo at Y = l_y, w_y * xo at Y = ny
 *     grad[(link * L + l_z) * 4 + c] += val * (1 - w_z);   grad[(link * L + l_z + 1) * 4 + c] += val * w_z
 *     (a term that is zero is not added);  mask[link * L + l_z] = mask[link * L + l_z + 1] = 1, whatever the terms
 * A ray left alone and a ray whose set-up is not finite contribute nothing; a ray that misses the box still crosses the
 * layers and does contribute. The adds are float atomics (one hardware add each, no compare-and-swap): two calls agree to
 * rounding of the sums, not bit for bit. mask_background may be NULL. sparsity_loss and beta_loss are not built
 * here (NERF_E_INVALID naming the feature): the foreground's share of both is nerf_grid_render_backward_losses', the
 * sparsity term of the background's own sigma samples exists nowhere. randomize is refused with the options.
 *
 * nerf_grid_background_tv_grad: for the `count` cells (start + i) mod (2R * R * L), i < count, of the [2R, R, L] volume (z
 * fastest) and each of the 4 channels c, on the background attached to the grid:
 *   v00 = the cell's value, v10 that of (nx, y, z), v01 that of (x, ny, z): both axes wrap; a texel without a row reads 0 and
 *   receives nothing. v_nxl = the value of layer z + 1 of the same texel; at the last layer, or without a row, it is 0 for
 *   sigma (c = 3) and v00 for the colours, and nothing is added at z + 1.
 *   dx = v10 - v00, dy = v01 - v00, dz = v_nxl - v00;  idelta = scale_c / sqrt(((1e-9 + dx dx) + dy dy) + dz dz), scale_c =
 *   scale_sigma for c = 3, else scale_color (the caller passes scaling / count);  dx *= 2R / 256, dy *= R / 256, dz *= L / 256
 *   grad[v00] += -((dx + dy) + dz) * idelta, grad[v_nxl] += dz * idelta, grad[v01] += dy * idelta, grad[v10] += dx * idelta
 * each only if the value added is not zero, and then the mask byte of that (row, layer) is set.
 *
 * nerf_grid_background_optim_step: nerf_grid_optim_step's arithmetic element for element (the same device function: its
 * NaN, subnormal, -0 and minval rules) over data [rows, 4], rows = capacity * L, in the rows whose mask byte is set, with
 * lr = lr_color for the columns 0..2 and lr_sigma for column 3 (svox2's lr_last). */
typedef struct nerf_grid_background_taped_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]                                                                */
    const float* dirs;          /* [dev] [n_rays, 3], need not be unit                                              */
    int64_t n_rays;             /* 0: nothing is done                                                               */
    float* rgb;                 /* [dev] [n_rays, 3] in / out                                                       */
    const float* log_transmit;  /* [dev] [n_rays]: the foreground's, not written                                    */
    float* log_transmit_out;    /* [dev] [n_rays] out, another array than log_transmit                              */
    double* tape;               /* [dev] [n_rays, 3] in / out: the foreground's tape                                */
    double* tape_background;    /* [dev] [n_rays, 3] out                                                            */
    void* stream;
} nerf_grid_background_taped_args;

typedef struct nerf_grid_background_backward_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]       (those of the taped pass)                                */
    const float* dirs;          /* [dev] [n_rays, 3]                                                                */
    int64_t n_rays;             /* 0: nothing is done                                                               */
    const float* grad_rgb;      /* [dev] [n_rays, 3] d loss / d rgb, contiguous                                     */
    const float* log_transmit;  /* [dev] [n_rays]: the foreground's, as the taped pass read it                      */
    const double* tape_background; /* [dev] [n_rays, 3] as the taped pass wrote it                                  */
    float* grad_background;     /* [dev] [capacity, L, 4], added to                                                 */
    uint8_t* mask_background;   /* [dev] [capacity, L] or NULL                                                      */
    float sparsity_loss;        /* must be 0 (not built)                                                            */
    float beta_loss;            /* must be 0 (not built)                                                            */
    void* stream;
} nerf_grid_background_backward_args;

typedef struct nerf_grid_background_tv_args {
    size_t struct_size;
    int64_t start, count;       /* cells (start + i) mod 2R R L; 0 <= start < 2R R L, 0 <= count <= 2R R L           */
    float scale_sigma;          /* finite                                                                           */
    float scale_color;          /* finite                                                                           */
    float* grad;                /* [dev] [capacity, L, 4], added to                                                 */
    uint8_t* mask;              /* [dev] [capacity, L]                                                              */
    void* stream;
} nerf_grid_background_tv_args;

typedef struct nerf_grid_background_optim_args {
    size_t struct_size;
    float* data;                /* [dev] [rows, 4], updated in place: background_data                               */
    float* rms;                 /* [dev] [rows, 4] (RMSProp; may be NULL for SGD)                                   */
    const float* grad;          /* [dev] [rows, 4]                                                                  */
    const uint8_t* mask;        /* [dev] [rows]                                                                     */
    int64_t rows;               /* capacity * L, in [0, 2^35]                                                       */
    int32_t kind;               /* NERF_GRID_OPTIM_RMSPROP / NERF_GRID_OPTIM_SGD                                    */
    float beta, lr_sigma, lr_color, eps, minval;
    void* stream;
} nerf_grid_background_optim_args;

int nerf_grid_background_rays_taped(nerf_sparse_grid* grid, const nerf_grid_render_options* opt,
                                    const nerf_grid_background_taped_args* args);
int nerf_grid_background_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* opt,
                                  const nerf_grid_background_backward_args* args);
int nerf_grid_background_tv_grad(nerf_sparse_grid* grid, const nerf_grid_background_tv_args* args);
int nerf_grid_background_optim_step(nerf_ctx* ctx, const nerf_grid_background_optim_args* args);

/* Sparse voxel grid: regularisers as values ---------------------------------------------------------
 * The regularisers of the Plenoxels objective as numbers with exact gradients: what a torch.autograd.Function needs so that
 * total variation and the sparsity term can be written into any loss (svox2's SparseGrid.tv() / tv_color(), and the function
 * whose gradient the sparsity_loss of nerf_grid_fused_backward_losses adds). The sections on training keep adding the
 * reference's gradients straight into a trainer's buffers; nothing there changes. All calls are stream-ordered, synchronise
 * and allocate nothing and return a status with nerf_last_error(). The backward calls ACCUMULATE: the caller zeroes.
 *
 * nerf_grid_tv_value: the total variation of the density table (target NERF_GRID_TV_DENSITY, one column) or of columns
 * [start_dim, end_dim) of the SH table (NERF_GRID_TV_SH; refused on a half-precision handle): svox2's tv_kernel. An item is
 * (cell, column c), a cell is a node (x, y, z) of the lattice. fp32, each operation one rounded operation, in this order:
 *   v0  = data[link(cell), c]  where the link is in [0, capacity), else 0
 *   v_i = the same at the +x, +y, +z neighbour; a neighbour that is empty or lies outside the lattice reads `null`:
 *         null = v0 with ignore_edge = 1 (its difference is 0), 0 with ignore_edge = 0
 *   with ignore_edge = 1 a cell whose own link is exactly row 0 contributes nothing (the reference's literal `links == 0`,
 *         as in nerf_grid_tv_grad_edge)
 *   d_i  = (v_i - v0) * s_i           s = (X / 256, Y / 256, Z / 256)
 *   term = sqrt(((1e-5 + dx dx) + dy dy) + dz dz)
 * *value = fp32(sum of term over cells and columns / n), the sum and the division in fp64, rounded once. svox2 runs tv() with
 * ignore_edge = 0 and tv_color() with 1. cells == NULL: the cells are the n = (X-1)(Y-1)(Z-1) nodes whose three forward
 * neighbours are inside the lattice, in C order (the reference's tv()). cells != NULL: n = n_cells flat C-order node
 * indices over X Y Z on the device, int32 or int64 (cells_int64), the stochastic form (svox2's _get_rand_cells): any node may
 * appear, repeatedly, and counts as often as it appears; an entry outside [0, X Y Z) contributes 0, stays in the divisor and
 * is never read through. n = 0 or start_dim == end_dim: *value = 0. The sum uses no float atomics: workgroup b adds the
 * terms of items [256 b, 256 b + 256) in fp64 in a fixed order into partials[b], and one workgroup adds the partials in a
 * fixed order: two calls on the same tables return the same bits. partials holds nerf_grid_tv_value_workspace(items)
 * doubles, items = n * (end_dim - start_dim) (1 column for the density): ceil(items / 256), 0 for items <= 0. Indices are
 * 64-bit throughout (2^30 nodes times 27 columns pass 2^32).
 *
 * nerf_grid_tv_value_backward adds to grad [capacity, columns of the table] the exact gradient of that value times the
 * cotangent grad_value[0], which the kernel reads from device memory. Per item, with the forward's d_i and term:
 *   w = grad_value[0] / fp32(n)
 *   neighbour i, if it is a kept row:  grad[row_i, c] += w * ((s_i * d_i) / term)
 *   the cell, if it is a kept row:     grad[row_0, c] += w * (-(((s_x dx) + (s_y dy)) + (s_z dz)) / term)
 * each unless the value added is 0 (a zero term is not added: a plateau of equal values receives exactly nothing). Float
 * atomics (one hardware add each): two calls agree to rounding of the sums. This is NOT svox2's
 * _TotalVariationFunction.backward, which calls tv_grad with a fixed scale of 1 (it ignores the cotangent), with 1e-9 where
 * the value has 1e-5, and with the rsqrt of the unscaled differences, which on a non-cubic lattice is the gradient of no
 * function; under autograd the gradient has to be that of the value returned. nerf_grid_tv_grad / nerf_grid_tv_grad_edge
 * keep the reference's literal rule.
 *
 * nerf_grid_sparsity_rays: sparsity[ray] = the sum of log1pf(2 (sigma sigma)) over the samples of the renderer's own march
 * (the lattice, step_size, near_clip, skip rule and stall rule of nerf_grid_render_rays) with sigma > opt.sigma_thresh, added
 * in fp32 in march order, up to and including the sample at which exp(log_T) < opt.stop_thresh ends the ray
 * (log_T = log_T + (-step_size * sigma) * delta_scale at every such sample, as in the renderer). A ray that is not marched
 * (a miss, a non-finite set-up) gives exactly 0. With skip data the result is bit-identical: a skipped sample has sigma = 0.
 * sh_data is not read. nerf_grid_sparsity_backward marches every ray again with the same log_T recurrence and adds to
 * grad_density the gradient of sum_ray grad_sparsity[ray] * sparsity[ray]: at every such sample
 *   d_sigma = grad_sparsity[ray] * ((4 sigma) / (1 + 2 (sigma sigma)))
 *   at each of the 8 corners whose link is kept:  v = ((w_x * w_y) * w_z) * d_sigma;  grad_density[row] += v  unless v == 0
 * (the expression nerf_grid_fused_backward_losses adds with sparsity_loss in the place of the cotangent). Nothing is kept
 * per ray between the two calls. At most 2^26 rays per call; n_rays = 0 does nothing. */
typedef struct nerf_grid_tv_value_args {
    size_t struct_size;
    int32_t target;             /* NERF_GRID_TV_DENSITY / NERF_GRID_TV_SH                                            */
    int32_t start_dim, end_dim; /* columns [start_dim, end_dim) of the table; the density has one: 0, 1              */
    int32_t ignore_edge;        /* 0 / 1                                                                            */
    const void* cells;          /* [dev] [n_cells] flat node indices, or NULL: every cell with three forward neighbours */
    int32_t cells_int64;        /* 0: cells are int32, 1: int64                                                     */
    int64_t n_cells;            /* with cells: in [0, 2^30]; ignored without                                        */
    double* partials;           /* [dev] [nerf_grid_tv_value_workspace(items)] workspace          (the value only)    */
    float* value;               /* [dev] [1] out                                                  (the value only)    */
    const float* grad_value;    /* [dev] [1] d loss / d value                                     (the backward only) */
    float* grad;                /* [dev] [capacity, columns of the table], added to               (the backward only) */
    void* stream;
} nerf_grid_tv_value_args;

typedef struct nerf_grid_sparsity_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]                                                                */
    const float* dirs;          /* [dev] [n_rays, 3], need not be unit                                              */
    int64_t n_rays;             /* 0: nothing is done                                                               */
    float* sparsity;            /* [dev] [n_rays] out                                             (the value only)    */
    const float* grad_sparsity; /* [dev] [n_rays] d loss / d sparsity                             (the backward only) */
    float* grad_density;        /* [dev] [capacity, 1], added to                                  (the backward only) */
    int32_t use_skip;           /* 1: use the skip data if nerf_grid_accelerate made it                             */
    void* stream;
} nerf_grid_sparsity_args;

int64_t nerf_grid_tv_value_workspace(int64_t items);
int nerf_grid_tv_value(nerf_sparse_grid* grid, const nerf_grid_tv_value_args* args);
int nerf_grid_tv_value_backward(nerf_sparse_grid* grid, const nerf_grid_tv_value_args* args);
int nerf_grid_sparsity_rays(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_sparsity_args* args);
int nerf_grid_sparsity_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_sparsity_args* args);

/* Sparse voxel grid: training data ------------------------------------------------------------------
 * A batch of training rays made from the images as they were loaded. svox2's DatasetBase.gen_rays materialises origin,
 * direction and colour of every pixel of every training image (36 B per ray) and shuffle_rays copies the whole set through a
 * host permutation once per epoch. Here the training set stays on the device as uint8 images and [n_images, 12] poses, and one
 * launch, one lane per ray, makes rows [begin, begin + n) of the epoch. The call is stateless, stream-ordered, allocates and
 * synchronises nothing and returns a status with nerf_last_error(). n == 0 launches nothing.
 *
 * Domain. h = height / factor, w = width / factor (integer division), N = n_images * h * w. A ray's index is
 * (image * h + y) * w + x, the reference's flattened rays_init. Output row k is the ray whose index is sigma(begin + k).
 *
 * sigma, by `order`. All arithmetic below is on unsigned 32-bit words (wrapping) unless it says 64-bit.
 *   hash32(v):  v ^= v >> 16;  v *= 0x7feb352d;  v ^= v >> 15;  v *= 0x846ca68b;  v ^= v >> 16
 *   round keys: klo = key & 0xffffffff, khi = key >> 32;  rk[r] = hash32(hash32(klo + r * 0x9e3779b9) ^ khi),  r = 0 .. 3
 *   NERF_GRID_ORDER_IDENTITY   sigma(p) = p                                                       (begin + n <= N)
 *   NERF_GRID_ORDER_PERMUTED   a bijection of [0, N)                                              (begin + n <= N)
 *     bits = the smallest even number >= 2 with 2^bits >= N;  half = bits / 2;  mask = 2^half - 1
 *     feistel(v), v < 2^bits:  L = v >> half, R = v & mask;  for r = 0 .. 3: (L, R) = (R, L ^ (hash32(R ^ rk[r]) & mask));
 *                              the result is (L << half) | R  (64-bit)
 *     sigma(p) = v = feistel(p); while v >= N: v = feistel(v)          (cycle walking)
 *     feistel is a bijection of [0, 2^bits), so the walk from p < N follows p's cycle and comes back into [0, N) at the latest
 *     at p itself: the loop ends, and sigma is a bijection of [0, N). 2^bits < 4 N, so a walk takes fewer than 4 steps on average.
 *   NERF_GRID_ORDER_RANDOM     independent draws, the reference's randint branch           (begin + n <= 2^62, any begin >= 0)
 *     plo = p & 0xffffffff, phi = p >> 32;  a = hash32(hash32(plo ^ rk[0]) ^ phi ^ rk[1]);  c = hash32(a ^ rk[2])
 *     sigma(p) = ((a << 32) | c) mod N                                                          (64-bit)
 *
 * Intrinsics. s = 1.0 / ((double)height / h) in fp64; fx' = (float)(fx * s), likewise fy', cx', cy' (svox2's Intrin.scale, whose
 * fp64 products PyTorch rounds to fp32 where they meet an fp32 tensor). Only the height enters s, as in the reference.
 *
 * Direction of pixel (x, y) of image i, fp32, every operation rounded separately, no fused multiply-add, true divisions:
 *   u = ((x + 0.5) - cx') / fx',  v = ((y + 0.5) - cy') / fy',  m = sqrt((u u + v v) + 1)
 *   (u, v, t) = (u / m, v / m, 1 / m)
 *   dirs[r] = (c2w[i][4 r] u + c2w[i][4 r + 1] v) + c2w[i][4 r + 2] t          r = 0, 1, 2;  c2w row-major [3, 4], OpenCV convention
 * origins[r] = c2w[i][4 r + 3], bit for bit.
 *
 * Colour of a full-resolution pixel, per channel c < 3, fp32: q_c = u8_c / 255 (a true division). With channels == 4 and
 * white_bkgd: a = u8_3 / 255 and q_c = (q_c a) + (1 - a). With channels == 4 and no white_bkgd the alpha is dropped.
 * factor == 1: rgb = q. factor > 1: the mean of q over rows [floor(y height / h), ceil((y + 1) height / h)) and columns
 * [floor(x width / w), ceil((x + 1) width / w)) (integer arithmetic; torch's interpolate(mode="area"), sizes that factor does
 * not divide included), summed in fp32 row by row, left to right, then divided by the number of pixels.
 *
 * Limits: 1 <= n_images <= 2^20, 1 <= height, width <= 2^15, channels 3 or 4, 1 <= factor <= min(height, width),
 * 0 <= n <= 2^26, fx and fy positive and finite, cx and cy finite. images must be 4-byte aligned when channels == 4. */
#define NERF_GRID_ORDER_IDENTITY 0
#define NERF_GRID_ORDER_PERMUTED 1
#define NERF_GRID_ORDER_RANDOM 2

typedef struct nerf_grid_dataset_batch_args {
    size_t struct_size;
    const uint8_t* images;      /* [dev] [n_images, height, width, channels]                                        */
    const float* c2w;           /* [dev] [n_images, 12]: rows 0..2 of the camera-to-world matrices                   */
    int32_t n_images, height, width, channels;
    double fx, fy, cx, cy;      /* of the full-resolution images                                                    */
    int32_t white_bkgd;
    int32_t factor;
    int32_t order;              /* NERF_GRID_ORDER_*                                                                */
    uint64_t key;               /* the epoch's key (unused by the identity order)                                   */
    int64_t begin, n;           /* rows [begin, begin + n) of the epoch                                             */
    float* origins;             /* [dev] [n, 3]                                                                     */
    float* dirs;                /* [dev] [n, 3]                                                                     */
    float* rgb;                 /* [dev] [n, 3]                                                                     */
    int64_t* indices;           /* [dev] [n] the ray index of every row, or NULL                                    */
    void* stream;
    float ndc_coeffs[2];        /* both > 0 (and finite): origin and direction above go through rays_to_ndc ("Sparse
                                   voxel grid", nerf_grid_camera), svox2's LLFFDataset.gen_rays; [0] <= 0 (a zeroed
                                   tail): world rays. The struct is 8 bytes larger than before this field was added    */
} nerf_grid_dataset_batch_args;

int nerf_grid_dataset_batch(nerf_ctx* ctx, const nerf_grid_dataset_batch_args* args);

/* Sparse voxel grid: surface meshes ----------------------------------------------------------------
 * A coloured triangle mesh of a grid's density field, on the grid's own lattice: no volume is resampled or materialised. Both
 * calls take a grid of nerf_grid_create, nerf_grid_create_half or nerf_grid_create_palette; background layers attached to it
 * are not read (they have no surface).
 *
 * The node value, for both calls. With p = (i, j, k) a node and n its C-order index:
 *     v(p) = density_data[links[n]]   where links[n] is in [0, capacity) and (mask == NULL or mask[n] != 0)
 *     v(p) = 0                        elsewhere: an empty node (any negative link) and a masked-out node
 * mask is [dev] uint8 [X, Y, Z]. Rows may be numbered in any order, two nodes may name one row, rows may be unreferenced.
 *
 * nerf_grid_marching_cubes: the isosurface v = iso. iso must be finite and > 0 (NERF_E_INVALID otherwise), so that an empty
 * node is outside. Every convention is nerf_marching_cubes' ("Mesh extraction": inside iff v >= iso and a NaN outside; one
 * welded vertex per crossing edge at t = (iso - a) / (b - a) in fp32, 0.5 when t is not finite; vertices in index coordinates
 * ordered by edge key, triangles by cell and table order; no atomics; both output pointers NULL = count only; a capacity too
 * small = NERF_E_INVALID, nothing written, the counts reported; `stream` is synchronised), and the result equals, in every bit
 * and in order, nerf_marching_cubes on the volume V[n] = v(p) with the same iso: the same kernels run with another source of
 * the node values. The passes read `links` as coalesced runs (and the mask's bytes beside them) and gather a density only
 * where a link is kept. The scratch is the context's workspace as for nerf_marching_cubes (nerf_workspace_bytes includes it:
 * 2 bytes per node and a few per 2048 nodes). A vertex in index coordinates x sits at the world position
 * center - radius + (x + 0.5) * 2 radius / reso ("Sparse voxel grid", Geometry).
 *
 * nerf_grid_mesh_attributes: normals and colours at n points given in index (grid) coordinates - the vertices above, or any
 * other points: a point cloud. A point's cell and weights are nerf_grid_sample's with grid_coords: x clamped to [0, reso - 1],
 * l = min(int(x), reso - 2), w = x - l, and every interpolation below is its trilinear one (z, then y, then x, fp32, each
 * operation rounded) over the 8 nodes of that cell. On a lattice edge all but two of the weights are zero, so a vertex needs
 * no record of its edge.
 *   Gradient. At a node q, G(q)_b = h_b (v(q + e_b) - v(q - e_b)) with a neighbour outside the lattice replaced by q itself,
 *     h_b = 0.5 where both neighbours exist and 1 at a border node. g = the interpolation of G at the point (index units).
 *   Normal. gw_b = g_b * scaling_b with scaling_b = reso_b / (2 radius_b) (the grid's own fp32 value), the gradient in world
 *     units; normal = -gw / |gw|, (0, 0, 0) where |gw| is 0 or not finite. -grad sigma points out of the region v >= iso:
 *     the side the triangles' right-hand normals face. |gw| is formed after dividing gw by its largest component.
 *   SH row. S[c][k], c < 3, k < basis_dim, is the interpolation of the rows' coefficients (an empty node is 0; the mask does
 *     not enter): bit for bit what nerf_grid_sample returns at the point, for each kind of grid from its own table.
 *   Colour, per channel c: clamp(0.5 + sum_{k < K} S[c][k] Y_k(d), 0, 1), Y the renderer's SH basis, the sum in order of k.
 *     NERF_GRID_MESH_COLOR_DC    K = 1 (Y_0 = 0.28209479177387814), no direction
 *     NERF_GRID_MESH_COLOR_SH    K = basis_dim, d = -normal: the ray that meets the surface head-on. Where the normal is
 *                                (0, 0, 0) the colour is NERF_GRID_MESH_COLOR_DC's.
 *     NERF_GRID_MESH_COLOR_VIEW  K = basis_dim, d = view, a unit vector (|view|^2 within 1e-5 of 1), the same for all points
 *     NERF_GRID_MESH_COLOR_NONE  no colours; `colors` must be NULL (and must not be with any other mode)
 *   normals may be NULL (not wanted). Stream-ordered, nothing is synchronised, no workspace. n <= 2^26. */
#define NERF_GRID_MESH_COLOR_NONE 0
#define NERF_GRID_MESH_COLOR_DC 1
#define NERF_GRID_MESH_COLOR_SH 2
#define NERF_GRID_MESH_COLOR_VIEW 3

typedef struct nerf_grid_mc_args {
    size_t struct_size;
    const uint8_t* mask;        /* [dev] [X, Y, Z] or NULL                                                          */
    float iso;                  /* finite, > 0                                                                      */
    float* vertices;            /* [dev] [vertex_capacity, 3] index coordinates, or NULL (count only)               */
    int64_t vertex_capacity;
    int64_t* triangles;         /* [dev] [triangle_capacity, 3] or NULL (count only)                                */
    int64_t triangle_capacity;
    int64_t* n_vertices;        /* [host] out                                                                       */
    int64_t* n_triangles;       /* [host] out                                                                       */
    void* stream;
} nerf_grid_mc_args;

typedef struct nerf_grid_mesh_attributes_args {
    size_t struct_size;
    const float* points;        /* [dev] [n, 3] index coordinates                                                   */
    int64_t n;
    const uint8_t* mask;        /* [dev] [X, Y, Z] or NULL: the mask of the extraction                              */
    int32_t color_mode;         /* NERF_GRID_MESH_COLOR_*                                                           */
    float view[3];              /* NERF_GRID_MESH_COLOR_VIEW: the unit direction                                    */
    float* normals;             /* [dev] [n, 3] or NULL                                                             */
    float* colors;              /* [dev] [n, 3] in [0, 1], or NULL with NERF_GRID_MESH_COLOR_NONE                   */
    void* stream;
} nerf_grid_mesh_attributes_args;

int nerf_grid_marching_cubes(nerf_sparse_grid* grid, const nerf_grid_mc_args* args);
int nerf_grid_mesh_attributes(nerf_sparse_grid* grid, const nerf_grid_mesh_attributes_args* args);

/* PlenOctree ----------------------------------------------------------------------------------------
 * An octree of branching factor 2 in svox's N3Tree layout, rendered by a cell-to-cell march. All arrays are borrowed.
 *   child  [dev] int32 [n, 2, 2, 2]     0: the cell is a leaf; else the child node's index minus this node's index (> 0)
 *   data   [dev] fp32  [n, 2, 2, 2, D]  D = 3 B + 1, B in {1, 4, 9, 16, 25}: a row is [R coefficients (B), G (B), B (B), sigma]
 * World to unit cube: x * invradius + offset. max_depth is the depth of the deepest node (the root has depth 0, at most 24);
 * a descent looks at no more than max_depth + 1 nodes, whatever `child` holds. nerf_octree_create checks every entry of
 * `child` on the device (0, or positive with node + entry < n; it synchronises `stream`), so that no descent leaves the arrays,
 * and that child, data and - in the render calls - every ray and output array are device memory of the context's GPU
 * (NERF_E_INVALID otherwise, before any launch).
 *
 * The march. svox is not part of the project this one was modelled on (it only calls into it), so the arithmetic is DEFINED
 * here: it restates svox 0.2's published algorithm from memory, it is not verified against svox. Every product, sum and
 * difference is one rounded fp32 operation in the order written; divisions are IEEE. min / max drop a NaN.
 *     o = origin * invradius + offset
 *     d = dir * invradius;  delta_scale = 1 / |d|  (|d| = sqrt((dx dx + dy dy) + dz dz));  d = d * delta_scale
 *     inv[i] = 1 / (d[i] + 1e-9)
 *     unit(p): t1 = -p[i] * inv[i];  t2 = t1 + inv[i];  tmin = max(0, min(t1, t2) over i);  tmax = min(1e9, max(t1, t2) over i)
 *     (tmin, tmax) = unit(o);  if tmax < 0 or tmin > tmax: rgb = background_brightness, steps = 0
 *     T = 1, t = tmin
 *     while t < tmax:
 *         p = clamp(o + t * d, 0, 1 - 1e-6)                   (1 - 1e-6: the fp32 difference of the fp32 constants)
 *         cube = 1, node = 0; repeat: p = p * 2; (u, v, w) = floor(p); p = p - (u, v, w); cube = cube * 2      (all exact)
 *                             until child[node][u][v][w] == 0 or max_depth + 1 nodes were looked at; else node += child[...]
 *         (a, b) = unit(p);  delta = (b - a) / cube + step_size                           (the division is exact)
 *         row = data[node][u][v][w];  sigma = row[D - 1]
 *         if sigma > sigma_thresh:
 *             att = exp((-delta * delta_scale) * sigma)
 *             s_c = sum over i < B, in order of i, of Y_i(viewdir) * row[c B + i]          c < 3
 *             rgb[c] = rgb[c] + (T * (1 - att)) * act(s_c);  T = T * att
 *             if T <= stop_thresh: rgb = rgb * (1 / (1 - T)); the ray ends here, without the background term
 *         if not (t + delta > t): leave the loop              (an origin so far away that the step is below one ulp of t)
 *         t = t + delta
 *     rgb[c] = rgb[c] + T * background_brightness
 * steps = the leaves looked at (passes through the loop). viewdir is the caller's direction as given (svox expects it
 * normalised); the image form makes its rays as nerf_grid_gen_rays does (unit directions), so nerf_octree_render_image equals
 * nerf_octree_render_rays on those rays bit for bit. act = 1 / (1 + exp(-s)) (NERF_OCTREE_RGB_SIGMOID, svox's) or
 * max(s + 0.5, 0) (NERF_OCTREE_RGB_RELU_HALF, svox2's colour model: what a tree built from a grid carries).
 * Y_i: the real spherical harmonics of degree 0..4 with the constants, signs and expressions of the reference's
 * plenoctree/nerf_sh/nerf/sh.py, each product and difference rounded, left to right, e.g. Y_12 = (C3[3] z) ((2 zz - 3 xx) - 3 yy).
 * A ray with a non-finite origin or direction component, or whose delta_scale is not finite and positive (a zero or an
 * overflowing direction), gets NaN in all channels and 0 steps. The loop ends after 65536 passes at the latest; the rays it
 * ended that way are added to *capped where that is not NULL.
 *
 * nerf_octree_accelerate: a dense table of side 2^k, k = min(levels, max_depth), built by one kernel and owned by the tree: an
 * entry holds the cell index and depth of the deepest cell of depth <= k that contains the table cell. Every later render starts
 * its descents at the entry of floor(p 2^k) instead of the root; with q = p 2^d the position inside a cell of depth d is
 * q - floor(q), which is the number the d exact doublings and subtractions of the plain descent give, so an accelerated render
 * equals a plain one bit for bit, steps included. levels in [0, 8]; 0, or a root-only tree, leaves the tree without a table.
 * Replacing or dropping a table waits for the device. nerf_octree_table_levels: k of the current table, 0 without one.
 *
 * nerf_octree_build_from_grid: svox2's SparseGrid.to_svox1 on the device, for a cubic fp32 grid (nerf_grid_create) of side
 * R = 2^L, 1 <= L <= 10. Leaf cell (i, j, k) at depth L holds [sh_data row, density] of lattice node (i, j, k) where
 * links >= 0 and zeros elsewhere; a cell above it has a child node exactly when a kept node lies under it, else it is a zero
 * leaf; the root always exists. Nodes are numbered breadth first: the root, then the nodes of depth 1 in C order of their
 * cell coordinates, then depth 2, ...: no atomics, two builds give the same bits. parent_depth[node] = (parent * 8 + u * 4 +
 * v * 2 + w, depth) of the cell the node hangs in; (0, 0) for the root (svox's value as remembered, not verified).
 * Two calls: with child == NULL the structure is planned into `workspace` (nerf_octree_build_workspace(R) bytes, 256-byte
 * aligned) and *n_nodes is written after ONE wait for `stream`; then, with the same workspace and arrays of n_nodes nodes,
 * the second call fills child, parent_depth and data, stream-ordered, waiting for nothing. The grid must not change between.
 *
 * PlenOctree: backward. nerf_octree_backward_rays / _image: the gradient of the march above with respect to the rows of
 * `data`, added to grad_data [n, 2, 2, 2, D] (fp32). Like the march, this arithmetic is defined here. The geometry of a march
 * (its leaves and their delta) depends on `child` and the ray alone, never on `data`, so a ray's colour is a smooth function
 * of the rows of the leaves it crosses, with fixed lengths. For one valid ray, in the notation above:
 *     the shaded leaves k = 1..m: those with sigma_k > sigma_thresh, in march order
 *     len_k = delta_k * delta_scale;  att_k = exp(-len_k sigma_k);  T_k: the transmittance before leaf k
 *     w_k = T_k (1 - att_k);  s_kc = sum_i Y_i row_k[c B + i];  col_kc = act(s_kc);  A_c = sum_k w_k col_kc
 *     T_e: the final transmittance;  stopped: T_e <= stop_thresh ended the march;  scale = 1 / (1 - T_e) if stopped, else 1
 *     U_c = A_c + (stopped ? 0 : T_e * background_brightness);  pre_kc = sum over j < k of w_j col_jc
 *     g_c: the incoming gradient of rgb_c;  act' = col (1 - col) for the sigmoid, (s + 0.5 > 0) ? 1 : 0 for relu_half
 *     d / d row_k[c B + i] += g_c * scale * w_k * act'(s_kc) * Y_i
 *     d / d sigma_k        += sum_c g_c * (scale * len_k * (T_k att_k col_kc - (U_c - pre_kc - w_k col_kc))
 *                                          + (stopped ? -A_c * scale^2 * len_k * T_e : 0))
 * The set of shaded leaves and the stopping leaf are held fixed (the function is piecewise smooth). Leaves at or below
 * sigma_thresh, leaves after the stop, rays that miss the cube and NaN rays get nothing. The call replays the march with
 * the renderer's operations: `rgb`, where not NULL, receives nerf_octree_render_rays' bits, and a ray that reaches the cap
 * of 65536 passes is added to *capped and contributes the gradient of the leaves it saw. The gradient itself is fp32
 * arithmetic in no promised order: float atomics arrive in any order, two calls may differ in the last bits. Adds of exact
 * zeros are skipped: a row no ray shaded is not touched.
 * Exactly one of grad_rgb and rgb_gt is given (NERF_E_INVALID otherwise). With grad_rgb [n, 3], g = grad_rgb. With rgb_gt
 * [n, 3], the fused clamped squared error: g_c = loss_scale * (clamp(rgb_c, 0, 1) - gt_c) where 0 <= rgb_c <= 1, else 0
 * (torch.clamp's closed interval), and *loss += sum over rays and c of (clamp(rgb_c, 0, 1) - gt_c)^2 where loss is not
 * NULL. A NaN ray adds nothing to either - a documented deviation: torch would give a NaN loss. loss_scale = 2 / (3 n)
 * makes grad_data the gradient of the mean squared error, and *loss / (3 n) that error.
 * The checks of the render calls (device memory of the context's GPU for every array given, n_rays <= 2^26, struct_size) come
 * before any launch. The table of nerf_octree_accelerate is honoured as in the renderer. The call waits for nothing. */
typedef struct nerf_octree nerf_octree;

#define NERF_OCTREE_RGB_SIGMOID 0
#define NERF_OCTREE_RGB_RELU_HALF 1
#define NERF_OCTREE_MAX_DEPTH 24

typedef struct nerf_octree_desc {
    size_t struct_size;
    int64_t n_nodes;            /* 1 .. 2^27                                                                        */
    int32_t data_dim;           /* 3 B + 1: 4, 13, 28, 49 or 76                                                     */
    int32_t max_depth;          /* 0 .. NERF_OCTREE_MAX_DEPTH                                                       */
    int32_t rgb_activation;     /* NERF_OCTREE_RGB_*                                                                */
    float invradius[3];         /* positive, finite                                                                 */
    float offset[3];            /* finite                                                                           */
    const int32_t* child;       /* [dev] [n_nodes, 2, 2, 2]                                                         */
    const float* data;          /* [dev] [n_nodes, 2, 2, 2, data_dim]                                               */
    void* stream;
} nerf_octree_desc;

typedef struct nerf_octree_render_options {
    size_t struct_size;
    float step_size;            /* > 0, finite; in units of the cube's side                                         */
    float sigma_thresh;         /* not NaN                                                                          */
    float stop_thresh;          /* not NaN                                                                          */
    float background_brightness;/* finite                                                                           */
} nerf_octree_render_options;

typedef struct nerf_octree_render_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]; unused by nerf_octree_render_image                            */
    const float* dirs;          /* [dev] [n_rays, 3]                                                                */
    int64_t n_rays;             /* 0 .. 2^26                                                                        */
    float* rgb;                 /* [dev] [n_rays, 3]                                                                */
    int32_t* steps;             /* [dev] [n_rays] or NULL                                                           */
    unsigned long long* capped; /* [dev] [1] added to, or NULL                                                      */
    void* stream;
} nerf_octree_render_args;

typedef struct nerf_octree_build_args {
    size_t struct_size;
    void* workspace;            /* [dev] nerf_octree_build_workspace(R) bytes                                       */
    int64_t workspace_bytes;
    int64_t* n_nodes;           /* [host] out of the planning call, in of the filling call                          */
    int32_t* child;             /* [dev] [n_nodes, 2, 2, 2], or NULL: plan                                          */
    int32_t* parent_depth;      /* [dev] [n_nodes, 2]                                                               */
    float* data;                /* [dev] [n_nodes, 2, 2, 2, 3 basis_dim + 1]                                        */
    void* stream;
} nerf_octree_build_args;

typedef struct nerf_octree_backward_args {
    size_t struct_size;
    const float* origins;       /* [dev] [n_rays, 3]; unused by nerf_octree_backward_image                          */
    const float* dirs;          /* [dev] [n_rays, 3]                                                                */
    int64_t n_rays;             /* 0 .. 2^26                                                                        */
    const float* grad_rgb;      /* [dev] [n_rays, 3], or NULL: exactly one of grad_rgb and rgb_gt                   */
    const float* rgb_gt;        /* [dev] [n_rays, 3], or NULL                                                       */
    float loss_scale;           /* finite; used with rgb_gt                                                         */
    float* grad_data;           /* [dev] [n_nodes, 2, 2, 2, data_dim], added to                                     */
    float* loss;                /* [dev] [1] added to (with rgb_gt), or NULL                                        */
    float* rgb;                 /* [dev] [n_rays, 3] out, or NULL                                                   */
    unsigned long long* capped; /* [dev] [1] added to, or NULL                                                      */
    void* stream;
} nerf_octree_backward_args;

int nerf_octree_create(nerf_ctx* ctx, const nerf_octree_desc* desc, nerf_octree** out);
void nerf_octree_destroy(nerf_octree* tree);
int nerf_octree_render_rays(nerf_octree* tree, const nerf_octree_render_options* opt, const nerf_octree_render_args* args);
int nerf_octree_render_image(nerf_octree* tree, const nerf_grid_camera* cam, const nerf_octree_render_options* opt,
                             const nerf_octree_render_args* args);
int nerf_octree_backward_rays(nerf_octree* tree, const nerf_octree_render_options* opt, const nerf_octree_backward_args* args);
int nerf_octree_backward_image(nerf_octree* tree, const nerf_grid_camera* cam, const nerf_octree_render_options* opt,
                               const nerf_octree_backward_args* args);
int nerf_octree_accelerate(nerf_octree* tree, int32_t levels, void* stream);
int nerf_octree_table_levels(const nerf_octree* tree);
int64_t nerf_octree_build_workspace(int32_t reso);      /* bytes, or -1 where reso is no power of two in [2, 1024] */
int nerf_octree_build_from_grid(nerf_sparse_grid* grid, const nerf_octree_build_args* args);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_H */
