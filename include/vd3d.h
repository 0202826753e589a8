/*
 * vd3d.h -- C ABI of libvd3d_hip.so: the MI355X (gfx950) depth-image-based stereo renderer.
 *
 * This is the drop-in boundary for ONE hot path of VisionDepth3D (reference tree
 * /root/reference, Python): the per-frame 2D->3D chain of core/render_3d.py.
 * The reference has no FFI; the boundary is a pair of Python call sites
 * (SURVEY.md 8(b)).  Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *  - plain C, no torch types.  All image pointers are DEVICE (HBM) pointers unless a
 *    name ends in _host.  Sizes are in pixels.  Planes are dense row-major.
 *  - "rgb_chw"  = float32 [3][h][w], R,G,B planes, values in [0,1]  (reference frame_to_tensor layout,
 *                 core/render_3d.py:135-138)
 *  - "bgr_hwc"  = uint8  [h][w][3], B,G,R interleaved                (OpenCV frame layout,
 *                 core/render_3d.py:289-291)
 *  - every call is ASYNCHRONOUS on the ctx's HIP stream and performs no host
 *    synchronisation; temporal-tracker scalars live in device memory inside the
 *    ctx and are advanced by a device-side scalar stage.  Use vd3d_sync() or
 *    vd3d_state_export() to observe results on the host.
 *  - return value: 0 on success, negative vd3d_status on error; vd3d_last_error()
 *    returns a thread-local message.
 */
#ifndef VD3D_H
#define VD3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6 (round 6): new entry points vd3d_gemm_x3_* / vd3d_attention_x3_* (no struct changed); vd3d_debug_tune answers only knobs 3 and 4 unless built with
 *    -DVD3D_DEV_KNOBS; aten_threads / aten_sum_threads accept 1 .. 1024.
 * 5 (round 5): vd3d_shift_params gained aten_threads / reserved0 at its end (vd3d_render_params embeds it: its later fields moved by 8 bytes); vd3d_torch_math_aten.
 * 4 (round 5): vd3d_render_params::reserved0 became aten_sum_threads (same layout).
 * Additions since 6 that leave the version as it is (no struct or existing signature changed): vd3d_depth_to_space_bias_nhwc_f32, vd3d_attention_f32, vd3d_attention_f32_form,
 *    the letterbox entry points (vd3d_letterbox_*, vd3d_canny_*, vd3d_depth_letterbox_fill_u8) with their two new structs, vd3d_conv3x3_s2_x3_weight_bytes,
 *    vd3d_conv3x3_s2_x3_pack_weights, vd3d_conv3x3_s2_x3, vd3d_patchify_f32 (DepthPipe(self_contained=True)), vd3d_depth_handoff_form, vd3d_depth_preprocess_form,
 *    vd3d_conv3x3_s1_x2_* and vd3d_conv3x3_s2_x2_* (weight_bytes, pack_weights and the convolution each: DepthPipe(conv="fp16x2")),
 *    vd3d_resize_pil_bicubic_u8, vd3d_depth_preprocess_pil (DepthPipe(front_end="pil")), vd3d_dpt_head_tail_act_f32 (the sigmoid tail of the metric
 *    Depth-Anything heads under DepthPipe(self_contained=True)), vd3d_im2col_nhwc_f32, vd3d_maxpool3x3_s2_nhwc_f32, vd3d_groupnorm_nhwc_f32_workspace_bytes and
 *    vd3d_groupnorm_nhwc_f32: the BiT prefix of DPT-Hybrid under DepthPipe(self_contained=True), vd3d_neck_poly_weight_bytes, vd3d_neck_poly_pack_f32 and
 *    vd3d_neck_poly_conv_f32 (the float32 neck's transposed convolution + 3 x 3 convolution in polyphase form), vd3d_depthpro_preprocess_u8
 *    and vd3d_depthpro_post_f32 (DepthPro's image-processor front end and post-process), vd3d_head_upconv_gather_f32 (the fine half of the float32 head's
 *    first convolution as coarse GEMM + fine gather), vd3d_head_conv_gather_weight_bytes, vd3d_head_conv_gather_tile, vd3d_head_conv_gather_pack_weights and
 *    vd3d_head_conv_gather_f32 (the float32 head's up-sampling + second convolution + tail as coarse GEMM + fine gather in one launch),
 *    vd3d_depthpro_patches_count, vd3d_depthpro_patches_f32 and vd3d_depthpro_merge_f32 (DepthPro's patch pyramid and patch merge: DepthPipe(encoders=...)),
 *    vd3d_conv3x3_epi (the stride-1 tile convolution with a residual unit's glue in its epilogue), vd3d_depthpro_head_weight_bytes,
 *    vd3d_depthpro_head_pack_weights and vd3d_depthpro_head (DepthPro's head behind its first convolution in one launch: DepthPipe(decoder=...)),
 *    vd3d_zoedepth_preprocess_u8, vd3d_zoedepth_post_f32, vd3d_zoedepth_attractor_f32 and vd3d_zoedepth_bins_f32 (ZoeDepth's image-processor ends and metric bin head). */
#define VD3D_ABI_VERSION 6

typedef enum vd3d_status {
  VD3D_OK = 0,
  VD3D_E_INVALID = -1,    /* bad argument (the reference raises AssertionError/ValueError) */
  VD3D_E_HIP = -2,        /* HIP runtime error */
  VD3D_E_NOMEM = -3,
  VD3D_E_UNSUPPORTED = -4 /* valid in the reference, not built yet here (fails loudly, never falls back) */
} vd3d_status;

/* output_format strings of format_3d_output, core/render_3d.py:837-860 */
typedef enum vd3d_format {
  VD3D_FMT_HALF_SBS = 0,
  VD3D_FMT_FULL_SBS = 1,
  VD3D_FMT_VR = 2,
  VD3D_FMT_ANAGLYPH = 3,
  VD3D_FMT_INTERLACED = 4
} vd3d_format;

/* depth input encodings accepted by vd3d_render_frame */
typedef enum vd3d_depth_fmt {
  VD3D_DEPTH_F32 = 0,     /* float32 [h][w] already in [0,1] (precomputed; BASELINE configs 1 and 3) */
  VD3D_DEPTH_BGR_U8 = 1,  /* uint8 [h][w][3] depth-video frame; depth_to_tensor, core/render_3d.py:140-143 */
  VD3D_DEPTH_GRAY_U8 = 2  /* uint8 [h][w]: same as BGR_U8 with B=G=R (BGR2GRAY is the identity on gray) */
} vd3d_depth_fmt;

/*
 * Keyword parameters of pixel_shift_cuda(), core/render_3d.py:561-590, same names,
 * same meaning, same defaults (vd3d_shift_params_default).  Python floats are doubles
 * and are narrowed to float32 at the same point torch narrows them.
 */
typedef struct vd3d_shift_params {
  double fg_shift, mg_shift, bg_shift;     /* positional args 5-7 */
  int32_t blur_ksize;                      /* 9   */
  int32_t use_subject_tracking;            /* 1   */
  int32_t enable_floating_window;          /* 1   */
  int32_t enable_feathering;               /* 1   */
  int32_t enable_edge_masking;             /* 1   */
  int32_t enable_dynamic_convergence;      /* 1   */
  double feather_strength;                 /* 10.0 */
  double max_pixel_shift_percent;          /* 0.02 */
  double parallax_balance;                 /* 0.8  */
  double zero_parallax_strength;           /* 0.0  */
  double convergence_strength;             /* 0.0  */
  double depth_pop_gamma;                  /* 0.85 */
  double depth_pop_mid;                    /* 0.50 */
  double depth_stretch_lo;                 /* 0.05 */
  double depth_stretch_hi;                 /* 0.95 */
  double fg_pop_multiplier;                /* 1.20 */
  double bg_push_multiplier;               /* 1.10 */
  double subject_lock_strength;            /* 1.00 */
  /* Extension, not a pixel_shift_cuda keyword (round 5).  N >= 1: reproduce ATen's SCALAR TAILS for a reference process that runs torch with N
   * intra-op threads (torch.get_num_threads()): torch.pow / torch.sigmoid on a float32 CPU plane split its n elements over min(N, ceil(n / 32768))
   * threads and send the last (chunk length mod 32) elements of every chunk through libm (std::pow in double with the unrounded Python exponent,
   * glibc's expf) instead of the SLEEF vector bodies (core/render_3d.py:209,517,620).  No plane a video produces has such a tail (1920x1080 and
   * 3840x2160 split evenly over 1 .. 96 threads); odd sizes do.  0 (the default): SLEEF values everywhere.  Inside vd3d_render_frame and the sharded entry
   * points vd3d_render_params::aten_sum_threads is used instead of this field.
   * HOST ISA ASSUMPTION of the mode (both fields): the reference's torch is an x86-64 build that dispatches to its AVX-512 kernels (elementwise loops step
   * two 16-lane vectors: tail = chunk length mod 32; an AVX2-only host would have mod 16) on glibc >= 2.27 (expf = the FMA ifunc variant, restated and checked
   * on all 2^32 inputs against glibc 2.35).  For a reference on another ISA the mode stays deterministic but is no longer that reference's bits at sizes with
   * tails.  Range 0 .. 1024.  The Python shims (pixel_shift_cuda, render_sbs_3d) pass torch.get_num_threads() of the calling process by default (round 6). */
  int32_t aten_threads;                    /* 0 */
  int32_t reserved0;
} vd3d_shift_params;

/*
 * Per-clip constants of the render_sbs_3d loop body, core/render_3d.py:1227-1419.
 * The geometry block is what lines 1074-1138 and 1236-1259 derive once per clip
 * (host helper: visiondepth3d_amd.geometry.plan_geometry mirrors them).
 */
typedef struct vd3d_render_params {
  /* geometry */
  int32_t src_w, src_h;          /* decoded frame size */
  int32_t crop_x, crop_y;        /* centre crop to the target aspect (:1236-1248) */
  int32_t crop_w, crop_h;
  int32_t eye_w, eye_h;          /* target_eye_w/h : size both tensors are resized to (:1250-1263) */
  int32_t warp_w, warp_h;        /* resized_width/height: size pixel_shift_cuda warps at (:1285) */
  int32_t fit_w, fit_h;          /* per_eye_w/h: size each eye is fitted to before muxing (:1409-1417) */
  int32_t out_w, out_h;          /* muxed frame size */
  int32_t format;                /* vd3d_format */
  int32_t auto_crop_black_bars;  /* :1230-1234: detect_black_bars + crop per frame, then the aspect crop of :1236-1248 is
                                    re-derived per frame ON DEVICE from target_ratio (crop_x/y/w/h are then ignored) */
  /* sliders */
  vd3d_shift_params shift;       /* fg/mg/bg are the UNSCALED slider values; dyn_scale/ipd are applied per frame */
  double ipd_factor;             /* :1283,1308 */
  double dof_strength;           /* max_sigma of apply_dof_cuda; 0 disables (:1340) */
  double sharpness_factor;       /* apply_sharpening factor (:1406) */
  double color_saturation, color_contrast, color_brightness; /* apply_color_grade (:1362-1365) */
  double target_ratio;           /* aspect_ratios[selected_aspect_ratio] (:1072); used when auto_crop_black_bars */
  /* Association of the DOF Gaussian levels (apply_dof_cuda -> torchvision gaussian_blur, core/render_3d.py:806).  The reference
   * blurs with a dense k x k depthwise convolution whose summation order belongs to the convolution library of the machine it
   * runs on.  1 (what vd3d_render_params_default sets): the dense convolution in the order PyTorch's CPU build (oneDNN) uses --
   * row-major taps, one fused multiply-add per tap -- which reproduces the CPU reference's blur BIT FOR BIT
   * (tests/test_oracle_vs_golden.py::test_b2_attribution*); fused into the finishing kernel.
   * 0: separable columns-then-rows sums -- 4x less arithmetic, identical to <= 6e-7 in float, which the reference's own uint8
   * truncation turns into +-1 LSB on ~0.5 % of samples before the sharpen stage (gain ~4.5): an opt-in fast mode. */
  int32_t dof_dense_conv;
  /* Float32 summation order of the two `torch.mean` calls on the path (compute_dynamic_parallax_scale :418, compute_motion_metric :928; round 5).
   * The reference's values are those of ATen's float32 cascade sum, which depends on the number of intra-op threads torch runs with
   * (TensorIterator splits reductions of >= 32 768 elements across them).  N >= 1: reproduce torch with N threads bit for bit
   * (torch.get_num_threads() of the reference process; its default is the machine's core count).  0 (what vd3d_render_params_default sets):
   * the correctly rounded mean of the exact sum -- independent of any thread count, within one float32 ULP of every N. */
  int32_t aten_sum_threads;                /* also the N of vd3d_shift_params::aten_threads for the frames of this clip */
} vd3d_render_params;

/*
 * All temporal-tracker scalars of the reference, made explicit (the reference keeps four of
 * them as never-reset module singletons, core/render_3d.py:284-285,500,511).
 */
typedef struct vd3d_state {
  /* FloatingWindowTracker :479-500 (alpha 0.97) */
  double fw_prev_offset;
  int32_t fw_frame_counter;
  /* DepthPercentileEMA :233-262 (float32 0-d tensors in the reference) */
  int32_t ema_valid;
  float ema_lo, ema_hi;
  /* ConvergenceEMA :273-280 (alpha 0.97) */
  int32_t conv_valid;
  int32_t bar_prev_width;        /* FloatingBarEaser :502-511 */
  double conv_val;
  /* FocalDepthTracker :895-922 */
  int32_t focal_valid;
  int32_t smooth_valid;          /* ShiftSmoother :463-477 */
  double focal;
  double sm_fg, sm_mg, sm_bg;
  /* plane state validity: TemporalDepthFilter.prev_depth (:220-229) and prev_depth_tensor (:1181,1463) */
  int32_t tdf_valid;
  int32_t prev_depth_valid;
} vd3d_state;

/* Per-frame scalars the device-side scalar stage produced (diagnostics, multi-GPU exchange, tests). */
typedef struct vd3d_frame_scalars {
  float q_lo, q_hi;              /* quantile(d,0.02/0.98) of the filtered depth (a5 inputs) */
  float ema_lo, ema_hi;          /* after the EMA */
  float mean_c, var_c;           /* centre-crop mean / unbiased variance (a6) */
  double dyn_scale;
  float s_norm;                  /* estimate_subject_depth(normalised eye-res depth): focal candidate, bar input */
  float mad;                     /* mean |d_t - d_{t-1}| (a15) */
  float s0, q05, q95, s1;        /* pixel_shift_cuda internals */
  float zpo_raw;                 /* zero-parallax offset before the tracker */
  double zpo;                    /* after FloatingWindowTracker */
  double focal;
  double stable_zero;
  int32_t bar_width;
  int32_t bar_side;              /* 0 none, 1 = mask right columns, 2 = mask left columns */
  int32_t collapse;              /* DepthPercentileEMA "hi-lo<1e-5" guard taken */
  int32_t crop_top, crop_bottom; /* detect_black_bars result of this frame (0,0 when auto crop is off) */
  int32_t reserved;
} vd3d_frame_scalars;

typedef struct vd3d_ctx vd3d_ctx;

/* ---- lifecycle -------------------------------------------------------------------------- */
int vd3d_abi_version(void);
const char* vd3d_last_error(void);
void vd3d_shift_params_default(vd3d_shift_params* p);   /* defaults of core/render_3d.py:569-589 */
void vd3d_render_params_default(vd3d_render_params* p);

/* One ctx per device per thread.  `stream` is a hipStream_t: NULL = the device's default (null) stream, which is
 * what PyTorch enqueues on by default, so tensors and vd3d calls stay ordered; VD3D_STREAM_PRIVATE = create and own a
 * private non-blocking stream (the caller then orders against it with events / vd3d_sync). */
#define VD3D_STREAM_PRIVATE ((void*)(intptr_t)-1)
int vd3d_ctx_create(int device, void* stream, vd3d_ctx** out);
int vd3d_ctx_destroy(vd3d_ctx* ctx);
int vd3d_sync(vd3d_ctx* ctx);                            /* hipStreamSynchronize */
/* The context's stream handle.  ESCAPE SEMANTICS: for a VD3D_STREAM_PRIVATE context the handle is from now on assumed to be held by the
 * caller (PyTorch wraps it and may record events on it when tensors marked with record_stream() are freed, possibly after the context
 * is gone), so vd3d_ctx_destroy no longer destroys that stream -- it is left to the process.  Query it once and keep it; a context whose
 * stream was never queried destroys it.  The same holds for vd3d_ctx_pixel_stream. */
void* vd3d_ctx_stream(vd3d_ctx* ctx);
/* re-target a context created on a caller-owned stream (not VD3D_STREAM_PRIVATE): later calls enqueue on `stream`, which is first
 * ordered behind everything the context has enqueued so far */
int vd3d_ctx_set_stream(vd3d_ctx* ctx, void* stream);
void* vd3d_ctx_pixel_stream(vd3d_ctx* ctx);              /* second stream of vd3d_set_pixel_overlap (NULL before it was enabled) */
void* vd3d_ctx_pixel_stream_k(vd3d_ctx* ctx, int k);     /* pixel stream k of vd3d_set_pixel_overlap(ctx, n), k < n <= 4 (k = 0: the one above) */

/* ---- tracker state (replaces the module singletons; lets ranks exchange it) -- */
int vd3d_state_reset(vd3d_ctx* ctx);                     /* fresh process + fresh render */
int vd3d_state_new_clip(vd3d_ctx* ctx);                  /* what render_sbs_3d re-creates per call (:1174-1182) */
int vd3d_state_export(vd3d_ctx* ctx, vd3d_state* host_out);      /* synchronises */
int vd3d_state_import(vd3d_ctx* ctx, const vd3d_state* host_in);
/* plane state: TemporalDepthFilter.prev_depth and prev_depth_tensor, float32 [eye_h][eye_w] device planes */
int vd3d_state_planes(vd3d_ctx* ctx, float** tdf_prev, float** norm_prev, int* eye_h, int* eye_w);
int vd3d_last_scalars(vd3d_ctx* ctx, vd3d_frame_scalars* host_out); /* synchronises */

/* ---- B1: pixel_shift_cuda, core/render_3d.py:561-712 --------------------------------------
 * rgb_chw [3][in_h][in_w] f32, depth [in_h][in_w] f32 (device) -> left/right bgr_hwc u8 [H][W][3]
 * (device), optional final_shift f32 [H][W].  Mutates the FloatingWindowTracker in ctx state
 * exactly as the reference mutates its module global (:651). */
int vd3d_pixel_shift(vd3d_ctx* ctx, const float* rgb_chw, const float* depth, int in_h, int in_w,
                     int W, int H, const vd3d_shift_params* p,
                     uint8_t* left_bgr, uint8_t* right_bgr, float* shift_or_null);

/* ---- B2: one iteration of the render_sbs_3d loop body, core/render_3d.py:1227-1419 ---------
 * frame_bgr u8 [src_h][src_w][3], depth per depth_fmt (device) -> out u8 [out_h][out_w][3] (device). */
int vd3d_render_frame(vd3d_ctx* ctx, const uint8_t* frame_bgr, const void* depth, int depth_fmt,
                      const vd3d_render_params* p, uint8_t* out_bgr);

/* The same loop iteration for a frame listed by skip_blank_frames (core/render_3d.py:1046-1060, branch :1278-1281): both eyes are
 * the raw source frame (source size), pixel_shift_cuda / ipd scaling / focal tracker / DOF / colour grade are skipped, the depth
 * filters, ShiftSmoother, dynamic scale and floating-window bars advance; sharpen, fit and mux run on the source-sized frame.
 * Which frames are blank is the caller's knowledge (the reference asks ffmpeg's blackdetect, core/ffmpeg_blackdetect.py:23-81). */
int vd3d_render_frame_blank(vd3d_ctx* ctx, const uint8_t* frame_bgr, const void* depth, int depth_fmt,
                            const vd3d_render_params* p, uint8_t* out_bgr);

/* ---- frame sharding: ONE clip over G GPUs, bit-identical to 1 GPU --------------------------------------------
 * The reference renders strictly frame by frame (core/render_3d.py:1194-1463); its temporal state is a plane EMA
 * (TemporalDepthFilter :220-229), a percentile EMA (:233-262) and non-linear scalar trackers (:463-511,895-922).  Here a "step" is
 * a window of n <= 512 consecutive frames cut into G contiguous chunks, one per rank.  Per step every rank runs
 *   [vd3d_tdf_plane_import]   the filtered plane of the frame before its chunk, received from the previous chunk's owner
 *                             (one eye-size float32 plane per chunk boundary, point to point);
 *   vd3d_shard2_p1            per own frame, in order: ingest + plane EMA + exact q.02 / q.98 of the filtered plane;
 *   [vd3d_tdf_plane_export]   the plane after its last frame, sent on to the next chunk's owner;
 *   all-gather of 2 floats per frame, vd3d_shard2_r1: DepthPercentileEMA replayed on every rank;
 *   vd3d_shard2_p3            per own frame: every other measurement (4 x int64 per frame), planes kept in the frame's slot;
 *   all-gather of 4 x int64 per frame, vd3d_shard2_r2: the remaining trackers replayed in frame order, own slots patched;
 *   vd3d_shard_pixels[_blank] per own frame: shift plane, warp, DOF, grade, sharpen, mux.
 * Data-path traffic per step and rank: <= 40 B per frame of records + one plane per chunk boundary. */
int vd3d_shard_begin(vd3d_ctx* ctx, const vd3d_render_params* p, int n_slots);
int vd3d_shard_pixels(vd3d_ctx* ctx, int slot, const vd3d_render_params* p, uint8_t* out_bgr);
/* the pixel pass of an own frame listed by skip_blank_frames (core/render_3d.py:1278-1281): both eyes are the source frame */
int vd3d_shard_pixels_blank(vd3d_ctx* ctx, int slot, const uint8_t* frame_bgr, const vd3d_render_params* p, uint8_t* out_bgr);
/* Overlapped pixel passes (no reference counterpart: the reference renders strictly frame by frame, core/render_3d.py:1194-1463).
 * enable != 0: vd3d_shard_pixels is enqueued on a second stream of the context, ordered after all work enqueued so far; the
 * measurement chain of the next step (vd3d_shard2_p1 .. r2; latency-bound scans) then overlaps the pixel kernels of this one.  A call
 * that overwrites a slot first waits for the pixel pass still reading it, so callers alternate between two slot sets to get the overlap.
 * Outputs are complete after vd3d_sync, or -- for consumers ordered on the context's stream -- after vd3d_join_pixels. */
/* enable = 0: off; 1: one pixel stream; 2 .. 4: consecutive pixel passes go round-robin over that many streams, each with its own shift
 * plane and warped eyes, so the kernels of neighbouring frames share the CUs (a consumer of the muxed frames orders itself behind
 * vd3d_join_pixels / vd3d_wait_pixels, or behind every vd3d_ctx_pixel_stream_k). */
int vd3d_set_pixel_overlap(vd3d_ctx* ctx, int enable);
int vd3d_join_pixels(vd3d_ctx* ctx);
int vd3d_wait_pixels(vd3d_ctx* ctx, int slot);   /* host waits for the outstanding overlapped pixel pass of `slot` (no-op if none) */

/* with auto_crop_black_bars: vd3d_shard2_p0 per own frame (crop rectangle {x,y,w,h} -> device int[4]), all-gather of the
 * rectangles, vd3d_shard2_set_crops(frame order) -- before vd3d_shard2_p1 of the step */
int vd3d_shard2_p0(vd3d_ctx* ctx, const uint8_t* frame_bgr, const vd3d_render_params* p, int* crop_out_dev);
int vd3d_shard2_set_crops(vd3d_ctx* ctx, const int* crops_all_dev, int n);
int vd3d_shard2_p1(vd3d_ctx* ctx, const uint8_t* frame_bgr, const void* depth, int depth_fmt,
                   const vd3d_render_params* p, int step_idx, int slot, float* q_out_dev);
/* TemporalDepthFilter.prev_depth (float32 [eye_h][eye_w]) out of / into the context: the chunk-boundary hand-off.  import with
 * valid = 0 installs "no previous frame" (what a fresh clip starts from). */
int vd3d_tdf_plane_export(vd3d_ctx* ctx, float* dst_dev, int eye_h, int eye_w);
int vd3d_tdf_plane_import(vd3d_ctx* ctx, const float* src_dev, int eye_h, int eye_w, int valid);
int vd3d_shard2_r1(vd3d_ctx* ctx, const float* q_all_dev, int n);
int vd3d_shard2_p3(vd3d_ctx* ctx, int slot, int step_idx, const vd3d_render_params* p, long long* m_out_dev);
/* Batched forms for the own frames of a step, which are consecutive (slots slot0 .. slot0 + n - 1, step indices step_idx0 ..,
 * n <= 16): P1 in two launches (the plane EMA -- a per-pixel recurrence of core/render_3d.py:225-229 -- walks the frames inside the
 * ingest kernel, the exact-quantile passes of the n frames run side by side), P3 in five launches for all n frames.  Same results
 * as n single calls; frames_bgr / depths are HOST arrays of n device pointers, q_out_dev = float[n][2], m_out_dev = int64[n][4]. */
int vd3d_shard2_p1_batch(vd3d_ctx* ctx, const uint8_t* const* frames_bgr, const void* const* depths, int depth_fmt,
                         const vd3d_render_params* p, int step_idx0, int slot0, int n, float* q_out_dev);
int vd3d_shard2_p3_batch(vd3d_ctx* ctx, int slot0, int step_idx0, int n, const vd3d_render_params* p, long long* m_out_dev);
/* blank_host_or_null[t] != 0: frame t of the step is in the skip_blank_frames set (no ipd scaling, no focal / FloatingWindowTracker
 * update for it, core/render_3d.py:1278-1281,1334-1337) */
int vd3d_shard2_r2(vd3d_ctx* ctx, const long long* m_all_dev, const int* own_slot_host, const uint8_t* blank_host_or_null, int n,
                   const vd3d_render_params* p);

/* ---- heal_missing_pixels(warped_frame, warped_depth, original_frame, edge_mask, heal_strength=0.5), core/render_3d.py:431-459 (a23):
 * the gradient-based hole fill.  warped_chw / original_chw / out_chw: float32 [3][H][W] (rgb_chw), edge_mask_or_null: float32 [H][W]
 * or NULL; the reference's warped_depth argument is unused by the reference and has no counterpart.  The reference's render
 * loop never calls this function, so it is an optional stage here too: callers that want it run it between B1 and the
 * finishing stage.  out may not alias the inputs. */
int vd3d_heal_missing_pixels(vd3d_ctx* ctx, const float* warped_chw, const float* original_chw, const float* edge_mask_or_null,
                             int H, int W, double heal_strength, float* out_chw);

/* ---- optional NV12 wire format at the frame I/O boundary.  The reference moves bgr24 (cv2.VideoCapture.read() in,
 * `ffmpeg -f rawvideo -pix_fmt bgr24` out, core/render_3d.py:987,1222,1143-1163,1422-1427) and leaves colour conversion to ffmpeg on
 * the host; with a decoder that emits NV12 and `-pix_fmt nv12` on the encoder pipe the wire carries 1.5 bytes per pixel and the
 * conversion runs on the frame already in HBM.  BT.601 limited range, 20-bit fixed point (OpenCV's cvtColor constants = swscale's
 * default matrix); no reference counterpart to be bit-exact with.  h and w even; pitches in bytes; uv_plane holds h/2 rows of
 * interleaved (U, V). */
int vd3d_nv12_to_bgr(vd3d_ctx* ctx, const uint8_t* y_plane, long long y_pitch, const uint8_t* uv_plane, long long uv_pitch, int h, int w,
                     uint8_t* out_bgr);
int vd3d_bgr_to_nv12(vd3d_ctx* ctx, const uint8_t* bgr, int h, int w, uint8_t* y_plane, long long y_pitch, uint8_t* uv_plane,
                     long long uv_pitch);

/* ---- cv2.resize(src, (dw, dh), interpolation=cv2.INTER_CUBIC) on uint8 images with cn = 1 or 3 interleaved channels: the resize of
 * the uint8 depth map back to the source size when the depth tab runs at an explicit inference size (a24,
 * core/render_depth.py:1914-1917) and the size changes of the up-scale stage (core/merged_pipeline.py:260-264).  OpenCV's
 * fixed-point bicubic (A = -0.75, 11-bit coefficients, replicate border, one rounding).  src != dst. */
int vd3d_resize_cubic_u8(vd3d_ctx* ctx, const uint8_t* src, int sh, int sw, int cn, uint8_t* dst, int dh, int dw);
/* cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) on uint8 BGR (3 interleaved channels): run_esrgan's input_res_pct < 100
 * (core/merged_pipeline.py:246-248) and pad_to_aspect_ratio (core/render_3d.py:121).  Down-scale ratios up to 10. */
int vd3d_resize_area_u8(vd3d_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, uint8_t* dst_bgr, int dh, int dw);
/* cv2.resize(src, (dw, dh)) with OpenCV's default interpolation (INTER_LINEAR, fixed point) on uint8 BGR: format_3d_output's VR branch */
int vd3d_resize_linear_u8(vd3d_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, uint8_t* dst_bgr, int dh, int dw);
/* format_3d_output(left, right, fmt) (core/render_3d.py:837-860) on two uint8 BGR eyes of h x w (device pointers).  out_bgr: [h][2 w][3] for the
 * SBS formats, [1600][2880][3] for VR (eyes of another size are resized with INTER_LINEAR first, like the reference), [h][w][3] for anaglyph
 * and interlaced. */
int vd3d_format_3d_output(vd3d_ctx* ctx, const uint8_t* left_bgr, const uint8_t* right_bgr, int h, int w, int format, uint8_t* out_bgr);

/* ---- up-scale stage glue (core/merged_pipeline.py:219-236).  The network between the two calls is the caller's
 * (visiondepth3d_amd.upscale runs it on PyTorch-ROCm).
 *   preprocess : preprocess_esr :219-223 -- BGR uint8 rows (pitch_bytes apart, so a tile crop needs no copy) -> RGB / 255 as
 *                float32, bf16 or fp16 (the reference's ONNX models are fp16), planar [3][h][w] or channels-last [h][w][3]
 *   postprocess: postprocess_esr :225-229 -- RGB float32 [h][w] planes (or channels-last) -> clip(0,1) * 255 truncated, BGR uint8;
 *                only the (cy, cx, ch, cw) window is written (the tile centre of _esrgan_tiled :266-284)
 *   add_weighted: blend_images :231-236 -- cv2.addWeighted(a, alpha, b, beta, gamma) on uint8 */
int vd3d_esr_preprocess(vd3d_ctx* ctx, int dtype, const uint8_t* frame_bgr, long long pitch_bytes, int h, int w, int channels_last,
                        void* out_rgb);
int vd3d_esr_postprocess(vd3d_ctx* ctx, const float* pred_rgb, int h, int w, int channels_last, int cy, int cx, int ch, int cw,
                         uint8_t* out_bgr, long long pitch_bytes);
int vd3d_add_weighted_u8(vd3d_ctx* ctx, const uint8_t* a, double alpha, const uint8_t* b, double beta, double gamma, long long n,
                         uint8_t* out);
/* run_rife's glue (core/merged_pipeline.py:195-218): concatenate_images + preprocess_rife -- two uint8 BGR frames / 255 stacked to six
 * channels in the frames' own order, float32 / bf16 / fp16, planar [6][h][w] or channels-last; and the output side -- float32
 * [3][h][w] (or channels-last) -> clip(0,1) * 255 truncated, channel order untouched.  The interpolation network between the two is
 * the caller's (the reference's RIFE ONNX graph is not in /root/reference). */
int vd3d_rife_preprocess(vd3d_ctx* ctx, int dtype, const uint8_t* frame1_bgr, const uint8_t* frame2_bgr, int h, int w, int channels_last,
                         void* out6);
int vd3d_rife_postprocess(vd3d_ctx* ctx, const float* pred3, int h, int w, int channels_last, uint8_t* out_bgr);

/* One body layer of the up-scale network on the matrix cores: y = PReLU(conv3x3(x, stride 1, zero padding 1) + bias), 64 -> 64 channels,
 * fp16 NHWC [H][W][64] in and out, float32 accumulate (v_mfma_f32_32x32x16_f16).  The reference runs these layers inside its ONNX
 * session (core/merged_pipeline.py:250-252); realesr-general-x4v3 has 32 of them.
 *   w_frag: the layer's weight Wt[oc][ic][kh][kw] pre-arranged in fragment order, fp16 [36 steps][2][64 lanes][8]:
 *           step = (kh*3 + kw)*4 + kc, element [step][t][l][j] = Wt[32 t + (l & 31)][16 kc + 8 (l >> 5) + j][kh][kw]
 *           (visiondepth3d_amd.upscale.conv_weight_fragments builds it)
 *   bias, slope_or_null: float32 [64] (slope NULL = no activation).  All pointers 16-byte aligned; x != y. */
int vd3d_conv3x3_c64_f16(vd3d_ctx* ctx, const void* x_nhwc, int H, int W, const void* w_frag, const float* bias, const float* slope_or_null,
                         void* y_nhwc);
/* The other two layers of the compact (SRVGG) networks the reference's model list holds (VisionDepth3D.py:1094-1098), also inside its ONNX
 * session (core/merged_pipeline.py:250-252):
 *   head: y = PReLU(conv3x3(x) + bias), 3 -> 64 channels, x fp16 NHWC [H][W][3] (vd3d_esr_preprocess, channels_last), y fp16 NHWC [H][W][64];
 *         w27x64: float32 [27][64], row (kh*3 + kw)*3 + ic, column oc = Wt[oc][ic][kh][kw]; float32 accumulate in that row order.
 *   tail: the 64 -> 3 r^2 convolution is vd3d_conv3x3_c64_f16 with weight fragments and bias zero-padded to 64 output channels and no activation;
 *         vd3d_esr_tail_f32 then applies pixel_shuffle(r) and adds the nearest-neighbour up-sampled input (the fp16 addition of the network)
 *         and writes the float32 planar prediction [3][r H][r W] that vd3d_esr_postprocess takes.  r = 2 or 4. */
int vd3d_conv3x3_head_f16(vd3d_ctx* ctx, const void* x_nhwc3, int H, int W, const float* w27x64, const float* bias, const float* slope_or_null,
                          void* y_nhwc64);
int vd3d_esr_tail_f32(vd3d_ctx* ctx, const void* t_nhwc64, const void* x_nhwc3, int H, int W, int r, float* out_planar);
/* The convolutions of RealESRGAN_x4plus (RRDBNet: 23 residual-in-residual dense blocks, 351 convolutions) on the matrix cores: 3x3, stride 1, zero
 * padding 1, fp16 operands, float32 accumulate (v_mfma_f32_32x32x16_f16), one fp16 rounding at the store.
 *   x: fp16 NHWC with a pixel stride of x_stride channels; channels [0, Cin) are read.  Cin: 64, 96, 128, 160 or 192.
 *   y: fp16 NHWC with a pixel stride of y_stride channels; the Cout (32 or 64) channels at [y_offset, y_offset + Cout) are written, nothing else.
 *      y may be the buffer x, provided the written slice does not meet [0, Cin): a dense block lives in one [H][W][192] buffer and needs no concatenation.
 *   w_frag: the weight Wt[oc][ic][kh][kw] in fragment order, fp16 [Cin/32 * 18 steps][Cout/32][64 lanes][8]:
 *           step = ((ic / 32)*9 + kh*3 + kw)*2 + kc, element [step][t][l][j] = Wt[32 t + (l & 31)][32 (ic / 32) + 16 kc + 8 (l >> 5) + j][kh][kw]
 *           (visiondepth3d_amd.upscale.dense_weight_fragments builds it).  The steps are accumulated in this order.  For a [64][64][3][3] weight this is
 *           NOT the order of vd3d_conv3x3_c64_f16 (tap-major there, 32-channel-chunk-major here).
 *   epilogue, in float32: v = acc + bias[oc]; v = v >= 0 ? v : v * slope (slope 1: no activation); if r1: v = v * alpha + r1[pixel][oc];
 *           if r2: v = v * beta + r2[pixel][oc].  r1 / r2: fp16 NHWC with pixel strides r1_stride / r2_stride (channels [0, Cout) are read), or NULL.
 *   up2: the input is [H/2][W/2] (H, W = the OUTPUT size, both even) and tap (gy, gx) reads its pixel (gy >> 1, gx >> 1) -- nearest x2 up-sampling
 *        folded into the convolution; padding is tested against H, W.  Built for Cin = Cout = 64.
 * Rules (VD3D_E_UNSUPPORTED with a message that names the broken one, nothing launched): the channel counts above; every stride and y_offset a multiple of 8,
 * x_stride >= Cin, y_offset + Cout <= y_stride, residual strides >= Cout; every pointer 16-byte aligned; the bytes written meet neither the bytes read
 * (an intersecting slice of the same buffer would be a race between workgroups) nor a residual.  One frame per call; bit-for-bit repeatable. */
int vd3d_conv3x3_dense_f16(vd3d_ctx* ctx, const void* x, int H, int W, int x_stride, int Cin, const void* w_frag, const float* bias, int Cout,
                           float slope, float alpha, const void* r1_or_null, int r1_stride, float beta, const void* r2_or_null, int r2_stride,
                           int up2, void* y, int y_stride, int y_offset);
/* The network's tail: channels 0..2 of an fp16 NHWC [H][W][32] map (conv_last on the kernel above, weights and bias zero-padded from 3 to 32 output
 * channels) -> the float32 planar prediction [3][H][W] that vd3d_esr_postprocess takes.  t 16-byte aligned. */
int vd3d_nhwc_f16_to_planar3_f32(vd3d_ctx* ctx, const void* t_nhwc32, int H, int W, float* out_planar);

/* ---- depth hand-off (a24): transformers' bicubic post-process to (H,W) + convert_depth_to_grayscale
 * (core/render_depth.py:585-611,1914-1916) for a batch of B predictions [B][ph][pw] float32 -> uint8 [B][H][W].
 * Replaces the reference's 8-bit depth video on disk while keeping its quantisation. */
int vd3d_depth_handoff(vd3d_ctx* ctx, const float* pred, int B, int ph, int pw, int H, int W, int invert, uint8_t* out_gray);
/* The same with the kernel named.  form 0: the library's choice (what vd3d_depth_handoff runs), 1: the general kernel (any size), 2: the separable
 * kernel, which keeps the horizontally interpolated prediction rows of a band of output rows in registers -- up-scaling only (ph <= H, pw <= W, not both
 * equal), VD3D_E_UNSUPPORTED elsewhere.  The forms give the same bytes. */
int vd3d_depth_handoff_form(vd3d_ctx* ctx, const float* pred, int B, int ph, int pw, int H, int W, int invert, uint8_t* out_gray, int form);

/* ---- tiled high-resolution depth (core/render_depth.py:62-66,102-194: infer_depth_tile, _normalize_to_u8).  The inference-size frame is cut into
 * `tile`-pixel tiles on a grid of core = max(1, tile - 2*pad), each cropped with a `pad` apron, resized so that both sides are multiples of 14, run
 * through the network, and the tile centres are blended under a Hann window; the hand-off is a 1 % - 99 % percentile normalisation.  All three
 * enqueue on the context's stream and do not synchronise; the tables are DEVICE arrays (visiondepth3d_amd/depth_tiles.py builds them).
 *
 * vd3d_tile_gather_cubic_u8: n apron crops of ONE size ch x cw -> out_tiles [n][chs][cws][3], each tile = cv2.resize(crop, (cws, chs), INTER_CUBIC)
 * bit for bit in vd3d_resize_cubic_u8's arithmetic (a copy when the sizes agree).  frames_bgr: B uint8 BGR frames of H x W, rows pitch_bytes and
 * frames frame_stride_bytes apart; origins_dev [n][3] int32 = (frame, y, x) of each crop (clamped into the batch by the kernel).  n <= 65535. */
int vd3d_tile_gather_cubic_u8(vd3d_ctx* ctx, const uint8_t* frames_bgr, long long pitch_bytes, long long frame_stride_bytes, int B, int H, int W,
                              const int32_t* origins_dev, int n, int ch, int cw, int chs, int cws, uint8_t* out_tiles);
/* vd3d_tile_blend_f32: out [B][tgt_h][tgt_w] = sum(centre * w) / max(sum(w), 1e-8) over the tiles that cover a pixel, added in row-major tile
 * order from 0 with separate multiply / add roundings (the reference's accumulation, bit for bit; no atomics).  Tile (ty, tx) of the
 * ceil(tgt_h / core) x ceil(tgt_w / core) grid has the entry tile_tab_dev[(ty * ntx + tx) * 8 ..] = {yc0, xc0, chs, cws, ph, pw, w_off, 0} (int32,
 * 16-byte aligned): its prediction for frame b is the float32 plane [ph][pw] at pred_pool + pred_off_dev[b * nt + t]; the centre sample of output
 * pixel (y, x) is element (yc0 + y - y0, xc0 + x - x0) of the chs x cws prediction -- read as is when (ph, pw) == (chs, cws), otherwise evaluated
 * with vd3d_depth_handoff's bicubic (align_corners=False) from the [ph][pw] plane; its weight is w_pool[w_off + (y - y0) * (x1 - x0) + (x - x0)].
 * Built for at most 4 covering tiles per axis (pad <= 3/8 tile): anything beyond returns VD3D_E_UNSUPPORTED and launches nothing. */
int vd3d_tile_blend_f32(vd3d_ctx* ctx, const float* pred_pool, const int64_t* pred_off_dev, const int32_t* tile_tab_dev, const float* w_pool,
                        int B, int tgt_h, int tgt_w, int tile, int pad, float* out);
/* vd3d_depth_normalize_pclip_u8: _normalize_to_u8 without its final resize, per frame of planes [B][H][W] float32 -> out_gray [B][H][W] uint8:
 * non-finite samples count as 0; lo / hi = numpy.percentile(d, p_lo / p_hi) (method "linear" on float32, exact order statistics by radix select);
 * hi - lo < 1e-6 -> min-max normalisation, or 128 everywhere when the range is below 1e-6 too; else clip((d - lo) / (hi - lo), 0, 1); * 255,
 * truncation, optional 255 - u8.  lo_hi_dev_or_null: [B][2] float32 device array that receives lo, hi (they never visit the host). */
int vd3d_depth_normalize_pclip_u8(vd3d_ctx* ctx, const float* planes, int B, int H, int W, float p_lo, float p_hi, int invert, uint8_t* out_gray,
                                  float* lo_hi_dev_or_null);

/* ---- letterbox handling of the depth pass (core/render_depth.py:280-573: LetterboxTracker and the detectors it calls; :1919-1933: the bar fill
 * behind the hand-off).  visiondepth3d_amd/letterbox.py holds the numpy statement these reproduce bit for bit (numpy's own arithmetic in numpy's
 * pairwise summation order; the cv2 parts -- BGR2GRAY, BGR2HSV's S, Canny, calcHist / normalize / compareHist, INTER_CUBIC -- from OpenCV's
 * documented 8-bit behaviour, unpinned).  Frames are dense uint8 BGR [B][H][W][3] in device memory, W <= 8192.  Everything enqueues on the
 * context's stream.  Host synchronisation: vd3d_letterbox_state_export / _import always; any other call only the FIRST time a context meets a
 * frame size or a larger batch (the summation plans of that size are built and uploaded with blocking copies and kept for the context's life -- none is evicted; lengths are at most 8192, a plan a few KB --,
 * workspaces grow behind a stream synchronise) -- steady state, alternating sizes included, enqueues and returns.  One tracker state per context. */
typedef struct vd3d_letterbox_state {   /* the reference tracker's attributes + what is_scene_cut compares the next frame with */
  int32_t top, bottom;                  /* the bars in force */
  int32_t locked_zero, locked_bars;
  int32_t cand_top, cand_bottom, streak;
  int32_t cooldown;                     /* frames left before a cut may re-measure */
  int32_t have_prev, prev_h, prev_w;    /* a previous frame's gray plane and 64-bin histogram are kept in the context */
  int32_t reserved;
} vd3d_letterbox_state;
typedef struct vd3d_letterbox_params {  /* LetterboxTracker.__init__ after its int() conversions */
  int32_t min_change, confirm_needed;
  int32_t max_total;                    /* int(h * max_total_frac) */
  int32_t cooldown_frames;              /* int(fps * cooldown_sec) */
} vd3d_letterbox_params;
/* vd3d_letterbox_stats: one pass over the frames.  Per row: float32 luma mean and variance (numpy's pairwise order) and the integer sum of the HSV
 * saturation (row_sat_sum [B][H] uint32; its mean is (float)sum / (float)W); the gray plane [B][H][W]; the 64-bin gray histogram [B][64] uint32;
 * mad_sum [B] uint64 = sum |gray_t - gray_(t-1)|; frame_mean [B] = y.mean() of the float32 luma plane.  Frame 0 has no predecessor (mad_sum 0) unless
 * chain != 0: then it is compared with the frame the tracker state keeps (when it has one of the same size), and the last frame of this batch
 * takes that place afterwards. */
int vd3d_letterbox_stats(vd3d_ctx* ctx, const uint8_t* frames_bgr, int B, int H, int W, int chain, float* row_mean, float* row_var,
                         uint32_t* row_sat_sum, uint8_t* gray, uint32_t* hist64, uint64_t* mad_sum, float* frame_mean);
/* vd3d_canny_u8: cv2.Canny(gray, low, high, apertureSize=3, L2gradient=True) per plane of gray [B][H][W] -> edges [B][H][W] (0 / 255);
 * row_counts_or_null [B][H] int32 receives the number of edge pixels per row.  vd3d_canny_hysteresis_u8 is its second half on a given class map
 * (0 none, 1 weak, 2 strong): 255 on every non-zero pixel that is 8-connected, through non-zero pixels, to a strong one. */
int vd3d_canny_u8(vd3d_ctx* ctx, const uint8_t* gray, int B, int H, int W, int low, int high, uint8_t* edges, int32_t* row_counts_or_null);
int vd3d_canny_hysteresis_u8(vd3d_ctx* ctx, const uint8_t* classes, int B, int H, int W, uint8_t* edges, int32_t* row_counts_or_null);
/* vd3d_letterbox_track: LetterboxTracker.update for the B frames of a step, in order, on the state in the context: statistics, Canny and one tracker
 * launch; out_bars [B][2] int32 = (top, bottom) in force after each frame (device memory). */
int vd3d_letterbox_track(vd3d_ctx* ctx, const uint8_t* frames_bgr, int B, int H, int W, const vd3d_letterbox_params* params, int32_t* out_bars);
/* Tracker state: reset = a new tracker (locked_zero, nothing kept); export / import move the scalars, and -- when the pointers are given and a
 * previous frame is kept -- its histogram (host, 64 uint32) and gray plane (DEVICE, prev_h * prev_w bytes; gray_capacity = room at prev_gray_dev).
 * An import without both pointers keeps no previous frame. */
int vd3d_letterbox_state_reset(vd3d_ctx* ctx);
int vd3d_letterbox_state_export(vd3d_ctx* ctx, vd3d_letterbox_state* out, uint32_t* prev_hist64_host_or_null, uint8_t* prev_gray_dev_or_null,
                                long long gray_capacity);
int vd3d_letterbox_state_import(vd3d_ctx* ctx, const vd3d_letterbox_state* in, const uint32_t* prev_hist64_host_or_null,
                                const uint8_t* prev_gray_dev_or_null);
/* vd3d_depth_letterbox_fill_u8: :1919-1933 per plane of depth [B][H][W] uint8 -> out (another buffer): (top, bottom) of frame b =
 * bars_dev[b * bars_stride + 0 / 1] (device int32; bars_stride 0 = one pair for all frames; negative values count as 0).  The plane is squeezed
 * into core_h = H - top - bottom rows with vd3d_resize_cubic_u8's arithmetic and the bar rows are filled with int(np.median(squeezed)); no bars, or
 * core_h <= 0, copy the plane. */
int vd3d_depth_letterbox_fill_u8(vd3d_ctx* ctx, const uint8_t* depth, int B, int H, int W, const int32_t* bars_dev, int bars_stride, uint8_t* out);

/* element type of the depth network's activations (a25).  The reference loads its Hugging Face depth models with
 * AutoModelForDepthEstimation.from_pretrained(checkpoint) and no dtype, i.e. float32 (core/render_depth.py:758-759,823-824):
 * VD3D_DT_F32 is the like-for-like precision, VD3D_DT_BF16 the optional reduced-precision mode. */
typedef enum vd3d_dtype { VD3D_DT_BF16 = 0, VD3D_DT_F32 = 1, VD3D_DT_F16 = 2 /* vd3d_esr_preprocess only */ } vd3d_dtype;

/* ---- depth-net input preparation (a25, core/render_depth.py:1106-1119 -> DPTImageProcessor): B uint8 BGR frames
 * [B][H][W][3] -> antialiased bicubic resize to (th,tw), 1/255, (x-mean)/std, RGB, `dtype`, NHWC [B][th][tw][3].
 * Returns VD3D_E_UNSUPPORTED when the down-scale factor exceeds the kernel's tap budget (scale > ~5.5). */
int vd3d_depth_preprocess(vd3d_ctx* ctx, const uint8_t* frames_bgr, int B, int H, int W, int th, int tw,
                          const float* mean3_host, const float* std3_host, int dtype, void* out_nhwc);
/* The same with the kernel named.  form 0: the library's choice (what vd3d_depth_preprocess runs), 1: the general tile kernel, 2: the strip kernel
 * (a workgroup filters a 32-column strip of a band of up to 32 output rows) -- down-scaling on both axes within its LDS plan (scale up to ~5.3),
 * VD3D_E_UNSUPPORTED elsewhere.  The forms give the same bits; a scale past the tap budget is VD3D_E_UNSUPPORTED whatever the form. */
int vd3d_depth_preprocess_form(vd3d_ctx* ctx, const uint8_t* frames_bgr, int B, int H, int W, int th, int tw,
                               const float* mean3_host, const float* std3_host, int dtype, void* out_nhwc, int form);

/* ---- the reference's own 8-bit input path, exact (DepthPipe(front_end="pil")).  The reference hands its depth pipeline PIL images: an optional
 * img.resize(inference_size, Image.BICUBIC) (core/render_depth.py:1113-1116) and the image processor's resize are both Pillow's ImagingResample on 8-bit
 * pixels, which rounds to uint8 after the horizontal and again after the vertical pass.  vd3d_resize_pil_bicubic_u8: B uint8 frames [B][H][W][3] ->
 * [B][h][w][3], channel order kept, the bytes Image.resize((w, h), Image.BICUBIC) gives (coefficients in double on the host, 22-bit fixed point, int32
 * sums; the horizontal pass only if the width changes, then the vertical pass only if the height changes; equal sizes copy).  Coefficient tables are
 * built at a geometry's first use (one blocking upload) and belong to the context.  VD3D_E_UNSUPPORTED, nothing launched, where an output index has
 * more than 24 taps (down-scales past ~5.5) or 32 output columns span more than 213 input pixels: visiondepth3d_amd/pil_resample.py states the same
 * operator for those. */
int vd3d_resize_pil_bicubic_u8(vd3d_ctx* ctx, const uint8_t* src, int B, int H, int W, uint8_t* dst, int h, int w);
/* The depth network's input from B uint8 BGR frames: that resize to (th, tw), BGR -> RGB, and the image processor's rescale and normalise as a table
 * of the byte, float32(float64(v) * (1 / 255)) then (x - mean) / std in float32 (rounded to bf16, nearest even, for VD3D_DT_BF16) -- NHWC
 * [B][th][tw][3] as vd3d_depth_preprocess writes it, equal to DPTImageProcessor's pixel_values bit for bit.  mid_h, mid_w > 0: the frames are first
 * resized to (mid_h, mid_w) by the uint8 form (the depth tab's inference size), a second launch; 0, 0: one launch.  VD3D_E_UNSUPPORTED as above if
 * either step is outside the plan. */
int vd3d_depth_preprocess_pil(vd3d_ctx* ctx, const uint8_t* frames_bgr, int B, int H, int W, int mid_h, int mid_w, int th, int tw,
                              const float* mean3_host, const float* std3_host, int dtype, void* out_nhwc);

/* Transformer-block glue of the depth network (a25): s = x + y, n = LayerNorm(s)*gamma + beta on [rows][cols] device arrays
 * of `dtype` in one pass (y == NULL: LayerNorm only, out_sum unused).  cols in {384, 768, 1024} (DA-V2 S/B/L), else
 * VD3D_E_UNSUPPORTED.  Replaces torch's add + layer_norm kernel pair inside DepthPipe's fused backbone. */
int vd3d_add_layernorm(vd3d_ctx* ctx, int dtype, const void* x, const void* y_or_null, const void* gamma, const void* beta,
                       float eps, int64_t rows, int cols, void* out_sum, void* out_norm);

/* The linear layers and the attention of the depth network's transformer blocks (a25; core/render_depth.py:1106-1119 runs them in float32 through the
 * Hugging Face pipeline) as SPLIT-operand GEMMs on the 16-bit matrix cores -- OPT-IN modes of DepthPipe (gemm="bf16x3" | "fp16x2"; the default stays
 * hipBLASLt's float32 GEMM + PyTorch's float32 attention).  gfx950 has no TF32 and its float32-input MFMA runs at 1/16 of the bf16 / fp16 rate.
 *   Y[M][N] = X[M][K] . W[N][K]^T + bias[N]   (row-major float32 device arrays, leading dimensions K / K / N; epilogue 1: + exact GELU)
 * mode VD3D_X3_BF16X3: every float32 operand is split EXACTLY into three bf16 terms (8 + 8 + 8 significant bits); six of the nine term products -- all but
 *   x2 w3, x3 w2, x3 w3, together <= 2^-23 |x w| -- go through v_mfma_f32_32x32x16_bf16 with float32 accumulation: float32-faithful (the error of a float32
 *   GEMM in another summation order; tests/test_hip_gemm.py vs float64 beside hipBLASLt), 6 MFMAs per MAC.  NaN / Inf inputs give NaN.
 * mode VD3D_X3_FP16X2: every operand as two fp16 terms, h1 = fp16(x), h2 = fp16(x - h1), round to nearest: 22 significant bits (|x - h1 - h2| <= 2^-22 |x|
 *   while h2 is a normal fp16 number, i.e. |x| >= 2^-2; below that the absolute error is <= 2^-25); three products x1 w1 + x1 w2 + x2 w1 -- HALF the matrix
 *   work.  Weight rows are pre-scaled by an exact power of two (undone in the epilogue) so that their second terms stay normal; activations are used as
 *   they are and must stay below 65 504 in magnitude (fp16's range; larger values give Inf / NaN).  Per product up to ~3 x 2^-22 relative instead of one
 *   float32 rounding; in a K >= 64 dot product that sits below the float32 accumulation error both modes share (measured beside hipBLASLt in the tests).
 * The weights are split and packed once: vd3d_gemm_x3_weight_bytes(N, K, mode) bytes (< 0: K is not a positive multiple of 16, or an unknown mode), filled
 * by vd3d_gemm_x3_pack_weights; the image is opaque, belongs to its mode and is only valid for this library version. */
enum { VD3D_GEMM_EPI_NONE = 0, VD3D_GEMM_EPI_GELU = 1 };
enum { VD3D_X3_BF16X3 = 0, VD3D_X3_FP16X2 = 1 };
int64_t vd3d_gemm_x3_weight_bytes(int N, int K, int mode);
int vd3d_gemm_x3_pack_weights(vd3d_ctx* ctx, const float* W, int N, int K, int mode, void* image);
int vd3d_gemm_x3(vd3d_ctx* ctx, const float* X, int64_t M, int K, const void* w_image, int N, int mode, const float* bias_or_null, int epilogue, float* Y);
/* The attention of the same blocks in the same arithmetic: out[b][t][h][:] = softmax_t'(q[b][t][h] . k[b][t'][h] * scale) v[b][t'][h] with
 * q / k / v = qkv[b][t][0 / 1 / 2][h][:], qkv the contiguous float32 output [B][T][3][H][D] of the fused QKV linear, out [B][T][H][D] float32.
 * Q, K, V and the probabilities are split like the GEMM operands of `mode` (fp16x2: q, k, v scaled by 2^4 and the probabilities by 2^10 before their split,
 * exactly, undone in the logits' scale and the final normalisation), both matrix products run on the matrix cores with float32 accumulation, the online
 * softmax is float32 (exp2 of the pre-scaled logits).  D = 64 only (every DINOv2 size), else VD3D_E_UNSUPPORTED.
 * Range: bf16x3 has float32's exponent.  In fp16x2 the 2^4 scale leaves |q|, |k|, |v| < 65 504 / 16 = 4 094: a larger value gives Inf / NaN in the outputs
 * that depend on it (a value: that column of its head; a key: its head) and nowhere else (tests/test_hip_operand_range.py).
 * `workspace`: vd3d_attention_x3_workspace_bytes(B, T, H, D, mode) bytes of device memory (the split images), 16-byte aligned, owned by the caller. */
int64_t vd3d_attention_x3_workspace_bytes(int B, int T, int H, int D, int mode);
int vd3d_attention_x3(vd3d_ctx* ctx, const float* qkv, int B, int T, int H, int D, float scale, int mode, void* workspace, int64_t workspace_bytes, float* out);
/* The same attention in exact float32 -- the default mode's (DepthPipe(gemm="f32")): both products on v_mfma_f32_32x32x2_f32 (float32 operands, float32
 * accumulation, bit for bit a k-ordered fmaf chain), float32 online softmax (exp2 of logits pre-scaled through q * (scale * log2 e)), one division by the
 * row sum at the end; nothing is rounded to a 16-bit format.  The arithmetic class of PyTorch's float32 scaled_dot_product_attention: only the summation
 * order and the exp implementation differ.  Same qkv / out layout as vd3d_attention_x3; no workspace.  VD3D_E_UNSUPPORTED for D != 64, an empty shape,
 * B * H > 65 535 or qkv / out not 16-byte aligned. */
int vd3d_attention_f32(vd3d_ctx* ctx, const float* qkv, int B, int T, int H, int D, float scale, float* out);
/* The same call with the kernel's form named: the workgroup's wave count, 8 (256 queries, one workgroup per CU) or 4 (128 queries, two per CU), or 0 = the
 * library's choice, which is what vd3d_attention_f32 passes.  Per query both forms run the same operations in the same order: their results are bit-identical,
 * the forms differ in speed only (tests, probes).  Any other form is VD3D_E_INVALID. */
int vd3d_attention_f32_form(vd3d_ctx* ctx, const float* qkv, int B, int T, int H, int D, float scale, float* out, int form);

/* The 3 x 3 convolutions of the DPT neck / head in the fp16x2 arithmetic (the third piece of DepthPipe(gemm="fp16x2")): stride 1, zero padding 1, no bias
 * (DepthPipe runs them bias-free with a glue launch behind each), float32 channels_last: X [B][H][W][Cin] -> Y [B][H][W][Cout], W the module's float32
 * weight [Cout][Cin][3][3].  Cin a multiple of 16, Cout 32, 64 or 128 (the fusion stage and the head's two 3 x 3 convolutions of DA-V2-Small / -Base), else
 * VD3D_E_UNSUPPORTED -- the caller keeps the library convolution for those.  Same arithmetic contract as vd3d_gemm_x3 in mode VD3D_X3_FP16X2 (operands as two
 * fp16 terms, three MFMA products, float32 accumulation, weights pre-scaled per output channel by an exact power of two, |x| < 65 504).
 * The weights are split and packed once into vd3d_conv3x3_x2_weight_bytes(Cin, Cout) bytes (< 0: unsupported shape). */
int64_t vd3d_conv3x3_x2_weight_bytes(int Cin, int Cout);
int vd3d_conv3x3_x2_pack_weights(vd3d_ctx* ctx, const float* W, int Cin, int Cout, void* image);
int vd3d_conv3x3_x2(vd3d_ctx* ctx, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y);
/* The same convolution (3 x 3, stride 1, zero padding 1, no bias, groups 1, float32 channels_last in and out) in the bf16x3 arithmetic of vd3d_gemm_x3 in mode
 * VD3D_X3_BF16X3 -- the convolutions of DepthPipe(gemm="bf16x3", conv="bf16x3"): every float32 operand is split EXACTLY into three bf16 terms by truncation
 * (8 + 8 + 8 significant bits); six of the nine term products go through v_mfma_f32_32x32x16_bf16, small products first (x1 w3, x3 w1, x2 w2, x1 w2, x2 w1,
 * x1 w1; x2 w3, x3 w2 and x3 w3 are dropped, as in the GEMM), float32 accumulation: float32-faithful (tests/test_hip_conv_x3.py vs float64).  bf16 has
 * float32's exponent: no weight pre-scaling and no activation range limit.  NaN / Inf inputs give NaN.
 * Cin a positive multiple of 16, Cout 32, 64, 128 or 256, H, W >= 1, 1 <= B <= 65 535, X and the image 16-byte aligned; anything else is VD3D_E_UNSUPPORTED
 * with a message that names the rule.  The weights are split and packed once into vd3d_conv3x3_x3_weight_bytes(Cin, Cout) bytes (host-only; < 0: shape not
 * built); the image is opaque and only valid for this library version. */
int64_t vd3d_conv3x3_x3_weight_bytes(int Cin, int Cout);
int vd3d_conv3x3_x3_pack_weights(vd3d_ctx* ctx, const float* W, int Cin, int Cout, void* image);
int vd3d_conv3x3_x3(vd3d_ctx* ctx, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y);
/* The stride-2 form for wide maps -- the reassemble stage's Conv2d(C, C, 3, stride 2, padding 1) of the DINOv2 depth models (C = 384 / 768 / 1024), the
 * convolution DepthPipe(self_contained=True) adds: no bias, groups 1, the same bf16x3 arithmetic (exact three-term truncation split, the six products above,
 * x1 w1 in one float32 accumulator and the five corrections in another, summed once), float32 NHWC in and out: X [B][H][W][Cin] -> Y [B][(H+1)/2][(W+1)/2][Cout],
 * W the module's float32 weight [Cout][Cin][3][3].  The kernel runs the space-to-depth view of the input and no tap on a zero weight, so a NaN / Inf input
 * pixel gives NaN in exactly the outputs whose 3 x 3 window holds it.  One fixed summation order per output (16-channel chunk, sub-pixel, tap; no split-K, no
 * atomics): bit-for-bit repeatable and independent of B.  128 output channels per workgroup; Cout = 128 n runs as n channel slices of the grid.
 * Cin a positive multiple of 16 (at most 65 536), Cout a positive multiple of 128 (at most 1024), H, W >= 1, 1 <= B <= 65 535, X and the image 16-byte aligned
 * (Y 4-byte); anything else is VD3D_E_UNSUPPORTED with a message that names the rule, and nothing is launched.  The weights are split and packed once into
 * vd3d_conv3x3_s2_x3_weight_bytes(Cin, Cout) bytes (host-only; < 0: shape not built): per slice, per 16 input channels, the K steps in the order a workgroup
 * runs them -- sub-pixel (0,0): tap (1,1); (0,1): (1,0), (1,2); (1,0): (0,1), (2,1); (1,1): (0,0), (0,2), (2,0), (2,2) -- then a 64-byte zero page.  The image
 * is opaque, differs from vd3d_conv3x3_x3's and is only valid for this library version. */
int64_t vd3d_conv3x3_s2_x3_weight_bytes(int Cin, int Cout);
int vd3d_conv3x3_s2_x3_pack_weights(vd3d_ctx* ctx, const float* W, int Cin, int Cout, void* image);
int vd3d_conv3x3_s2_x3(vd3d_ctx* ctx, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y);
/* The two tile convolutions above in the fp16x2 arithmetic of vd3d_gemm_x3 in mode VD3D_X3_FP16X2 -- the convolutions of DepthPipe(gemm="fp16x2",
 * conv="fp16x2"): the same kernel plan (8 x 32 output tile, every channel count and map size the bf16x3 forms take), the same layouts and rules.
 *   vd3d_conv3x3_s1_x2  3 x 3, stride 1, zero padding 1: X [B][H][W][Cin] -> Y [B][H][W][Cout], Cout 32, 64, 128 or 256 (256 as two slices of 128).
 *   vd3d_conv3x3_s2_x2  3 x 3, stride 2, zero padding 1: X [B][H][W][Cin] -> Y [B][(H+1)/2][(W+1)/2][Cout], Cout a positive multiple of 128, at most 1024; the
 *                       space-to-depth view with no tap on a zero weight, so a non-finite input reaches exactly the outputs whose window holds it.
 * No bias, groups 1, float32 NHWC in and out, W the module's float32 weight [Cout][Cin][3][3].  Cin a positive multiple of 16 (at most 65 536), H, W >= 1,
 * 1 <= B <= 65 535, X and the image 16-byte aligned (Y 4-byte); anything else is VD3D_E_UNSUPPORTED with a message that names the rule, and nothing is launched.
 * Arithmetic contract: 22 significant bits per operand.  x ~ h1 + h2 with h1 = fp16(x), h2 = fp16(x - h1), both round to nearest; the weights of output channel
 * oc are scaled by 2^e(oc), e = 13 - floor(log2 max |W[oc]|) clamped to [-100, 100] (0 for an all-zero or non-finite channel), and split the same way into g1 + g2,
 * so that second terms stay normal fp16 numbers.  Three products per MAC on v_mfma_f32_32x32x16_f16: h1 g1 into one float32 accumulator, h1 g2 and h2 g1 into a
 * second one; h2 g2 is dropped.  The two are summed once and multiplied by 2^-e (exact).  One fixed summation order per output (16-channel chunk, then tap): bit for
 * bit repeatable and independent of B.  Range: |x| < 65 504; a larger |x|, Inf or NaN makes every output whose window holds it Inf / NaN over all channels -- never a
 * finite wrong number -- and touches no other output.  |x| below 2^-14 loses its second term gradually (fp16 subnormals are kept, not flushed): the absolute
 * error per operand stays <= 2^-25.
 * Weight image, vd3d_conv3x3_s{1,2}_x2_weight_bytes(Cin, Cout) = (Cin / 16) * 9 * Cout * 64 + 4 * Cout + 64 bytes (host-only; < 0: shape not built):
 *   [slice Cout / CK][K step 9 Cin / 16][term 2][k-half 2][oc CK][8 fp16], CK = min(Cout, 128), K step = (16-channel chunk, tap) in the order a workgroup runs
 *   them (stride 1: taps row-major; stride 2: the sub-pixel order of vd3d_conv3x3_s2_x3), channel 16 chunk + 8 k-half + element;
 *   then colscale[Cout] = 2^-e as float32; then a 64-byte zero page.  The image is only valid for this library version. */
int64_t vd3d_conv3x3_s1_x2_weight_bytes(int Cin, int Cout);
int vd3d_conv3x3_s1_x2_pack_weights(vd3d_ctx* ctx, const float* W, int Cin, int Cout, void* image);
int vd3d_conv3x3_s1_x2(vd3d_ctx* ctx, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y);
int64_t vd3d_conv3x3_s2_x2_weight_bytes(int Cin, int Cout);
int vd3d_conv3x3_s2_x2_pack_weights(vd3d_ctx* ctx, const float* W, int Cin, int Cout, void* image);
int vd3d_conv3x3_s2_x2(vd3d_ctx* ctx, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y);
/* The stride-1 tile convolution with the glue of a pre-activation residual unit in its epilogue -- the residual units and head.layers.0 of
 * DepthPipe("depth-pro", decoder=...): 3 x 3, stride 1, zero padding 1, float32 NHWC, X [B][H][W][Cin] -> Y (and Yrelu) [B][H][W][Cout], in the arithmetic of
 * `mode`: VD3D_X3_BF16X3 reads the image of vd3d_conv3x3_x3_pack_weights, VD3D_X3_FP16X2 the image of vd3d_conv3x3_s1_x2_pack_weights (no image format of its
 * own).  In this order, every step one float32 operation (the library is built without contraction):
 *   u = the bare sum exactly as vd3d_conv3x3_x3 / vd3d_conv3x3_s1_x2 forms it (same tile, K order and accumulators: acc + lo, times colscale in fp16x2) over X --
 *       with VD3D_EPI_RELU_IN over (x != x ? x : max(x, 0)), applied to the staged pixels in front of the split: a NaN stays a NaN;
 *   v = u;  bias != NULL: v = v + bias[oc];  r1 != NULL: v = v + r1[p][oc];  r2 != NULL: v = r2[p][oc] + v;  VD3D_EPI_RELU: v = max(v, 0);
 *   Y[p][oc] = v;  Yrelu != NULL: Yrelu[p][oc] = max(v, 0).
 * That is vd3d_nhwc_bias_act_f32's chain: Y and Yrelu EQUAL, bit for bit, what [relu ->] the bias-free convolution -> vd3d_nhwc_bias_act_f32 writes
 * (tests/test_hip_conv_epi_bits.py), without the bare sum and the ReLU'd input ever reaching memory.  max(NaN, 0) is 0 there and here.  The range and NaN
 * contract of each mode is the bias-free entry point's; bit for bit repeatable and independent of B.
 * Rules (VD3D_E_UNSUPPORTED with a message that names the broken one, nothing launched, nothing written): Cin a positive multiple of 16 (fp16x2: at most
 * 65 536), Cout 32, 64, 128 or 256; H, W >= 1; 1 <= B <= 65 535; X and the image 16-byte aligned, bias / r1 / r2 / Y / Yrelu 4-byte; r1 and r2 are dense
 * [B][H][W][Cout] maps; Y and Yrelu overlap neither X, r1, r2, the bias, the image nor each other (a workgroup reads the halo its neighbours' tiles would
 * write).  A mode or a flag bit outside the above is VD3D_E_INVALID. */
/* Everything behind head.layers.0 of DepthProDepthEstimationHead as ONE launch on the coarse map (DepthPipe("depth-pro", decoder=...)), in the arithmetic of
 * `mode` (VD3D_X3_BF16X3 | VD3D_X3_FP16X2, the contracts of the tile convolutions above):
 *   ConvTranspose2d(Cin, Cin, 2, 2) + bt -> Conv2d(Cin, 32, 3, padding 1) + b2 -> ReLU -> Conv2d(32, 1, 1) + b3 -> ReLU:  x [B][h][w][Cin] -> out [B][2h][2w]
 * The transposed convolution and the 3 x 3 convolution are one linear map: per output phase (p_y, p_x) four taps on the coarse grid (offsets p - 1 and p per
 * axis), the tap geometry of VD3D_IFN_T4S2.  Wc [16][32][Cin] holds the composed blocks, block (2 p_y + p_x) * 4 + 2 t_y + t_x for tap offset
 * (p_y + t_y - 1, p_x + t_x - 1): Wc[k] = sum of W3[:, :, dy, dx] @ Wt[:, :, (p_y + dy) & 1, (p_x + dx) & 1]^T over the fine taps that land in the offset
 * (visiondepth3d_amd.depth.neck_poly_compose(wt, None, w3, 2): float64, rounded once).  The 3 x 3 convolution pads the FINE map with zeros, not with bt, so
 * the constant term is a table T [3][3][32] indexed by (first / interior / last fine row, likewise the column):
 * T = b2 + sum of W3[:, :, dy, dx] @ bt over the taps whose fine pixel is inside the map (float64 on the host, rounded once).  Per output pixel, in float32:
 *   v[oc] = acc + lo (times colscale[oc] in fp16x2) over the taps, 16-channel chunk then tap;  u[oc] = max(v[oc] + T[row class][column class][oc], 0);
 *   d = sum over oc of w3[oc] * u[oc] as a butterfly over the 32 channels (partner distance 16, 8, 4, 2, 1, in that order);  out = max(d + b3, 0).
 * max(NaN, 0) is 0, as in vd3d_dpt_head_tail_f32.  No split-K, no atomics: bit for bit repeatable and independent of B.  Neither 2h x 2w x Cin map exists.
 * The blocks are split and packed once into vd3d_depthpro_head_weight_bytes(mode, Cin) bytes (host-only; < 0: not built): [phase 4][chunk Cin / 16][tap 4] K
 * steps of [term][k-half 2][oc 32][8] (bf16x3: three exact terms; fp16x2: two terms of 2^e W with e per output channel over all 16 blocks, then colscale[32]),
 * then a 64-byte zero page; the image belongs to its mode and is only valid for this library version.
 * Rules (VD3D_E_UNSUPPORTED with a message that names the broken one, nothing launched, nothing written): Cin a positive multiple of 16 (at most 65 536);
 * 1 <= B <= 65 535; 1 <= h, w <= 16 384; x and the image 16-byte aligned, Wc / T / w3 / out 4-byte; out does not overlap x.  Any other mode: VD3D_E_INVALID. */
int64_t vd3d_depthpro_head_weight_bytes(int mode, int Cin);
int vd3d_depthpro_head_pack_weights(vd3d_ctx* ctx, int mode, const float* Wc, int Cin, void* image);
int vd3d_depthpro_head(vd3d_ctx* ctx, int mode, const float* x, int B, int h, int w, int Cin, const void* w_image, const float* T, const float* w3, float b3,
                       float* out);
enum { VD3D_EPI_RELU_IN = 1, VD3D_EPI_RELU = 2 };
int vd3d_conv3x3_epi(vd3d_ctx* ctx, int mode, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, int flags,
                     const float* bias_or_null, const float* r1_or_null, const float* r2_or_null, float* Y, float* Yrelu_or_null);

/* The convolutions of the RIFE interpolation network (IFNet HDv3; RifeSession(conv="bf16x3")) in the same bf16x3 arithmetic: exact three-term truncation
 * split of every float32 operand, the products x1 w3, x3 w1, x2 w2, x1 w2, x2 w1 into one float32 accumulator and x1 w1 into another, summed in the epilogue
 * (v_mfma_f32_32x32x16_bf16).  Float32 NHWC in and out, NaN / Inf inputs give NaN, no range limit, bit-for-bit repeatable.
 *   kind VD3D_IFN_K3S1: Conv2d(3, stride 1, padding 1), output H x W.            W: [Cout][Cin][3][3]
 *   kind VD3D_IFN_K3S2: Conv2d(3, stride 2, padding 1), output (H+1)/2 x (W+1)/2. W: [Cout][Cin][3][3]
 *   kind VD3D_IFN_T4S2: ConvTranspose2d(4, stride 2, padding 1), output 2H x 2W, computed as four output phases of 2 x 2 taps.  W: [Cin][Cout][4][4]
 *   X: pixels of pitch x_stride floats, channels [0, Cin) are read, Cin a positive multiple of 16.  H x W is the INPUT size, B frames.
 *   Y: pixels of pitch y_stride floats, the Cout (32, 64 or 96) channels at [y_offset, y_offset + Cout) are written, nothing else.  A network with other
 *      channel counts pads weights, bias and slopes with zeros (visiondepth3d_amd.rife does: 11 / 45 / 90 -> 16 / 64 / 96).
 *   epilogue, in float32: v = acc + lo + bias[oc]; slope != NULL: v = v >= 0 ? v : slope[oc] * v (per-channel PReLU); r != NULL: v += r[pixel][oc], r being
 *      output-sized pixels of pitch r_stride.
 * Rules (VD3D_E_UNSUPPORTED with a message that names the broken one, nothing launched): the kinds and channel counts above; 1 <= B <= 65 535; H, W >= 1;
 * x_stride a multiple of 4 and >= Cin; y_stride >= y_offset + Cout, y_offset >= 0; r_stride >= Cout; X and the image 16-byte aligned, bias / slope / r / Y
 * 4-byte aligned; the bytes written meet neither the bytes read (a slice of the same buffer that intersects channels [0, Cin) would be a race between
 * workgroups) nor the residual.  The weights are split and packed once into vd3d_conv_ifn_weight_bytes(kind, Cin, Cout) bytes (host-only; < 0: not built);
 * the image is opaque, belongs to its kind and is only valid for this library version. */
enum { VD3D_IFN_K3S1 = 0, VD3D_IFN_K3S2 = 1, VD3D_IFN_T4S2 = 2 };
int64_t vd3d_conv_ifn_weight_bytes(int kind, int Cin, int Cout);
int vd3d_conv_ifn_pack_weights(vd3d_ctx* ctx, int kind, const float* W, int Cin, int Cout, void* image);
int vd3d_conv_ifn(vd3d_ctx* ctx, int kind, const float* X, int B, int H, int W, int x_stride, int Cin, const void* w_image, const float* bias,
                  const float* slope_or_null, int Cout, const float* r_or_null, int r_stride, float* Y, int y_stride, int y_offset);
/* The float32 glue between the blocks of that network.  x6: the network input, planar [N][6][h][w] (frame 0, frame 1, in [0, 1]); the network works on
 * Hp x Wp = h, w rounded up to multiples of 32, the padding reads as 0.  state: NHWC [N][Hp][Wp][8] = running flow (4), mask (1), zeros (3).
 * "warp" = grid_sample(bilinear, padding_mode="border", align_corners=True) of a frame at pixel + flow, computed in pixel units (sample position clamped to
 * [0, Wp-1] x [0, Hp-1]).  scale in {1, 2, 4}; N <= 65 535; every pointer 16-byte aligned.
 *   vd3d_rife_warp_pack: a block's input, NHWC [N][Hp/scale][Wp/scale][16] = F.interpolate(scale_factor=1/scale, bilinear, align_corners=False) of
 *      [warp(frame 0, flow[0:2]) (3), warp(frame 1, flow[2:4]) (3), mask (1), flow / scale (4)], then 5 zeros.  The down-scale is the mean of the centre 2 x 2
 *      pixels of each cell.  state_or_null == NULL: flow and mask are zero (the first block).
 *   vd3d_rife_update: flow += up(t[..][0:4]) * scale, mask += up(t[..][4]), up = F.interpolate(scale_factor=scale, bilinear, align_corners=False);
 *      t: NHWC [N][Hp/scale][Wp/scale] pixels of pitch t_stride >= 5 (a multiple of 4).  first != 0: the state is written, not added to.
 *   vd3d_rife_blend: out planar [N][3][h][w] = warp(frame 0) * m + warp(frame 1) * (1 - m), m = sigmoid(mask): what vd3d_rife_postprocess takes. */
int vd3d_rife_warp_pack(vd3d_ctx* ctx, const float* x6, const float* state_or_null, int N, int h, int w, int scale, float* out16);
int vd3d_rife_update(vd3d_ctx* ctx, const float* t, int t_stride, int first, int N, int h, int w, int scale, float* state);
int vd3d_rife_blend(vd3d_ctx* ctx, const float* x6, const float* state, int N, int h, int w, float* out);

/* F.interpolate(mode="bilinear", align_corners=True) of an NHWC (channels_last) tensor [B][ih][iw][C] -> [B][oh][ow][C] of
 * `dtype`, C a multiple of 8 (bf16) / 4 (f32): the up-samplings of the DPT neck / head (a25). */
int vd3d_upsample_bilinear_nhwc(vd3d_ctx* ctx, int dtype, const void* in, void* out, int B, int ih, int iw, int oh, int ow, int C);

/* Float32 glue between the library convolutions of the DPT neck / head (a25; transformers DepthAnythingPreActResidualLayer /
 * FeatureFusionLayer / DepthEstimationHead as the reference's pipeline runs them, core/render_depth.py:1106-1119).  NHWC maps of n_pix
 * pixels x C channels (C a multiple of 4).
 *   vd3d_nhwc_bias_act_f32:  v = y [+ bias[c]] [+ r1]; [v = r2 + v]; [v = max(v, 0)] -> out (may alias y); [relu_out = max(v, 0)]
 *   vd3d_upsample_bilinear_bias_nhwc_f32:  vd3d_upsample_bilinear_nhwc + bias[c] on the interpolated value (up(conv + b) == up(conv) + b)
 *   vd3d_dpt_head_tail_f32:  out[p] = max(b3 + sum_c w3[c] * max(y[p][c] + b2[c], 0), 0) * scale -- conv2's bias, ReLU, the 1x1 conv3, its
 *                            bias, the final ReLU and max_depth of the head in one pass; C in {16, 32, 64}
 *   vd3d_dpt_head_tail_act_f32:  the same pass with the head's last activation as an argument:
 *                                  v = b3 + sum_c w3[c] * max(y[p][c] + b2[c], 0)
 *                                  act VD3D_HEAD_ACT_RELU    (0): out[p] = max(v, 0) * scale    -- vd3d_dpt_head_tail_f32's function, the same bits
 *                                  act VD3D_HEAD_ACT_SIGMOID (1): out[p] = sigmoid(v) * scale   -- the metric Depth-Anything heads (Sigmoid() * max_depth)
 *                                v is formed exactly as vd3d_dpt_head_tail_f32 forms it (same lanes, same FMA chain, same butterfly).  sigmoid is
 *                                torch.sigmoid on a float32 CPU tensor, 1 / (1 + Sleef_expf_u10(0 - v)) -- what vd3d_torch_math(op 1) returns; the sigmoid and
 *                                the multiplication by scale are two float32 roundings, as in the module graph.
 * Both tails: y, b2 and w3 16-byte aligned, C in {16, 32, 64} (else VD3D_E_UNSUPPORTED); n_pix >= 1 and, for the second, act in {0, 1} (else
 * VD3D_E_INVALID).  A refused call launches nothing and leaves out as it was. */
enum { VD3D_HEAD_ACT_RELU = 0, VD3D_HEAD_ACT_SIGMOID = 1 };
int vd3d_nhwc_bias_act_f32(vd3d_ctx* ctx, const float* y, const float* bias_or_null, const float* r1_or_null, const float* r2_or_null, int relu,
                           int64_t n_pix, int C, float* out, float* relu_out_or_null);
int vd3d_upsample_bilinear_bias_nhwc_f32(vd3d_ctx* ctx, const float* in, const float* bias, float* out, int B, int ih, int iw, int oh, int ow, int C);
int vd3d_dpt_head_tail_f32(vd3d_ctx* ctx, const float* y, const float* b2, const float* w3, float b3, float scale, int64_t n_pix, int C, float* out);
int vd3d_dpt_head_tail_act_f32(vd3d_ctx* ctx, const float* y, const float* b2, const float* w3, float b3, float scale, int64_t n_pix, int C, int act, float* out);

/* The DPT head's 3 x 3 convolution with its up-sampling in front and, optionally, the tail behind, in one exact-float32 kernel (float32 operands on
 * v_mfma_f32_32x32x2_f32, float32 accumulation, one fixed K order -- 16-channel chunk, tap, channel -- no split-K, no atomics: identical from run to run):
 *     y = conv3x3(up(x) + b_in)     x float32 NHWC [B][ih][iw][Cin]; up = bilinear, align_corners=True, to [oh][ow]: bit for bit what
 *                                   vd3d_upsample_bilinear_bias_nhwc_f32 writes (ih == oh && iw == ow: the identity); zero padding 1, stride 1, no bias
 *     b2, w3 given:  out[B][oh][ow]       = max(b3 + sum_c w3[c] * max(y[c] + b2[c], 0), 0) * scale      (vd3d_dpt_head_tail_f32's function)
 *     b2, w3 NULL:   out[B][oh][ow][Cout] = y
 * The intermediate maps of the three launches it replaces are never written.  Built: Cin 32 | 64 | 128 -> Cout 32 with the tail, Cin 128 -> Cout 64 plain;
 * 1 <= B <= 65 535, oh, ow >= 2; x, b_in, the image, b2, w3 and a plain output 16-byte aligned.  Anything else is VD3D_E_UNSUPPORTED and nothing is launched.
 * The weights [Cout][Cin][3][3] are packed once into vd3d_dpt_head_conv_weight_bytes(Cin, Cout) bytes (host-only; < 0: shape not built):
 * [chunk Cin / 16][tap 9][quad 4][oc Cout][4 floats]. */
int64_t vd3d_dpt_head_conv_weight_bytes(int Cin, int Cout);
int vd3d_dpt_head_conv_pack_weights(vd3d_ctx* ctx, const float* W, int Cin, int Cout, void* image);
int vd3d_dpt_head_conv_f32(vd3d_ctx* ctx, const float* x, const float* b_in, int B, int ih, int iw, int oh, int ow, int Cin, const void* w_image, int Cout,
                           const float* b2_or_null, const float* w3_or_null, float b3, float scale, float* out);

/* The neck's ConvTranspose2d(C, C, kernel_size=f, stride=f) with bias and the bias-free 3 x 3 / padding 1 convolution behind it as ONE exact-float32 kernel on the
 * coarse map (v_mfma_f32_32x32x2_f32, float32 accumulation, no split-K, no atomics: a frame's bits depend neither on the batch nor on the call):
 *     out[b][f i + pa][f j + pb][:] = sum_k Wc[k] x[b][i + di_k][j + dj_k][:] + sum_k bc[k]     over the blocks k of phase (pa, pb) whose coarse pixel is inside the map
 * x float32 NHWC [B][h][w][Cin] -> out float32 NHWC [B][f h][f w][Cout]; the fine map between the two layers is never written.  Blocks: phases (pa, pb) row-major,
 * inside a phase di ascending, then dj ascending; phase coordinate 0 reaches offsets {-1, 0}, f - 1 reaches {0, 1}, any other {0}: (f + 2)^2 blocks.  The caller
 * composes Wc [block][Cout][Cin] and bc [block][Cout] (float32, contiguous) from the two layers' parameters; vd3d_neck_poly_pack_f32 lays Wc out for the kernel in
 * vd3d_neck_poly_weight_bytes(Cin, Cout, f) bytes (host-only; < 0: shape not built): [block][slot Cin / KS][step KS / 8][k-half 2][oc Cout][4 floats], KS = 32 (16 where
 * Cin is no multiple of 32), channel slot KS + k-half KS / 2 + 4 step + e.  Built: (Cin, Cout, f) = (96, 128, 4), (192, 128, 2), (48, 64, 4), (96, 64, 2); every pointer
 * 16-byte aligned; anything else is VD3D_E_UNSUPPORTED and nothing is launched. */
int64_t vd3d_neck_poly_weight_bytes(int Cin, int Cout, int f);
int vd3d_neck_poly_pack_f32(vd3d_ctx* ctx, const float* Wc, int Cin, int Cout, int f, void* image);
int vd3d_neck_poly_conv_f32(vd3d_ctx* ctx, const float* x, int B, int h, int w, int Cin, const void* w_image, const float* bc, int Cout, int f, float* out);

/* The fine half of conv3x3(upsample_bilinear(conv1x1(x) + b_p)) (the last fusion layer's projection, the align_corners up-sampling and the head's bias-free 3 x 3 /
 * padding 1 convolution: all linear, so all channel mixing is ONE GEMM on the coarse map, Z[b][i][j][t][o] = sum_c (W_t P)[o][c] x[b][i][j][c] + (W_t b_p)[o] for
 * the 9 taps t = 3 ky + kx, which the caller runs):
 *     out[b][Y][X][o] = sum over t = 0 .. 8 ascending with (Y + ky - 1, X + kx - 1) inside [0, H) x [0, W) of bilinear(Z[b][:][:][t][o]; Y + ky - 1, X + kx - 1)
 * Z float32 [B][h][w][9][Cout] -> out float32 NHWC [B][H][W][Cout], the convolution WITHOUT its bias.  Coordinates as vd3d_upsample_bilinear_nhwc's float32 path
 * (s = (float)(h - 1) / (float)(H - 1), f = s * (float)y, truncation, the < h - 1 clamp, l1 = f - (float)i0, l0 = 1.f - l1); per tap the corner weights ly * lx are
 * rounded products and every value is one fmaf chain from 0 in the order taps ascending, corners (y0, x0), (y0, x1), (y1, x0), (y1, x1), summed by one lane: no
 * atomics, bits depend neither on the batch nor on the call.  Built: Cout = 64 | 32; H, W >= 2 (any size, not only 2 h x 2 w; a down-sampling factor above about
 * 9 is refused); both pointers 16-byte aligned; anything else is VD3D_E_UNSUPPORTED and nothing is launched. */
int vd3d_head_upconv_gather_f32(vd3d_ctx* ctx, const float* z, int B, int h, int w, int H, int W, int Cout, float* out);

/* vd3d_dpt_head_conv_f32's function with the tail -- out[B][oh][ow] = max(b3 + sum_o w3[o] * max(conv3x3(up(y1 + b1))[o] + b2[o], 0), 0) * scale, Cin -> 32 channels --
 * in "coarse GEMM + fine gather" form, one launch: conv3x3(up(y1 + b1)) = sum over the 9 taps t = 3 ky + kx of S_t up(W_t y1 + W_t b1), so all channel mixing runs
 * on the COARSE map (float32 operands on v_mfma_f32_32x32x2_f32) and the fine map keeps 36 multiply-adds per value; Z is produced and consumed in LDS.
 *     y1 float32 NHWC [B][ih][iw][Cin] (conv1 WITHOUT its bias); Wt the tap-major weight [9 x 32][Cin], row t 32 + o = W[o][:][ky][kx]; bc [9][32],
 *     bc[t][o] = sum_c W[o][c][ky][kx] b1[c] (the caller composes both); b2, w3 [32].
 * Arithmetic: Z_t[p][o] is one fmaf chain from 0 over the channels in the order q = 0 .. Cin / 8 - 1, j = 0 .. 3: channel 8 q + j, then 8 q + 4 + j; then + bc[t][o].
 * A fine value a[o] is one chain acc = fmaf(w, z, acc) from 0 over the taps ascending whose fine position is inside the map (a tap outside contributes nothing,
 * bias included), corners (y0, x0), (y0, x1), (y1, x0), (y1, x1), weights the rounded products ly * lx of vd3d_upsample_bilinear_nhwc's float32 coordinates
 * (vd3d_head_upconv_gather_f32's order); the tail is s = fmaf(max(a[o] + b2[o], 0), w3[o], s) from 0 for o ascending, out = max(s + b3, 0) * scale.  No split-K, no
 * atomics: bits depend neither on the batch nor on the call.  Association differs from vd3d_dpt_head_conv_f32 (which samples x and adds b): close, not equal bits.
 * vd3d_head_conv_gather_pack_weights lays Wt out in vd3d_head_conv_gather_weight_bytes(Cin) bytes (host-only; < 0: not built): [tap 9][q Cin / 8][lane 64][4 floats],
 * lane = 32 kh + o holding channels 8 q + 4 kh + 0 .. 3 of output channel o.  vd3d_head_conv_gather_tile (host-only) reports the fine tile th x tw the launch would
 * cut the map into.  Built: Cin 32 | 64 | 128; oh, ow >= 2 (any size; a down-sampling factor above about 6 is refused); y1, Wt, the image, bc, b2, w3 16-byte
 * aligned.  Anything else is VD3D_E_UNSUPPORTED and nothing is launched. */
int64_t vd3d_head_conv_gather_weight_bytes(int Cin);
int vd3d_head_conv_gather_tile(int ih, int iw, int oh, int ow, int Cin, int* th, int* tw);
int vd3d_head_conv_gather_pack_weights(vd3d_ctx* ctx, const float* Wt, int Cin, void* image);
int vd3d_head_conv_gather_f32(vd3d_ctx* ctx, const float* y1, int B, int ih, int iw, int oh, int ow, int Cin, const void* w_image, const float* bc, const float* b2,
                              const float* w3, float b3, float scale, float* out);

/* The reassemble stage's transposed convolutions of DPT-Large (DPTReassembleLayer.resize = ConvTranspose2d(C, C, kernel_size=s, stride=s, padding=0), s = 4 / 2):
 * kernel == stride, so the windows do not overlap and the layer is a GEMM Y[p][(i, j, co)] = sum_ci X[p][ci] W[ci][co][i][j] (vd3d_gemm_x3 with the weight
 * permuted to [(i, j, co)][ci]) followed by this scatter: y [P = B*H*W][s][s][C] float32 -> out NHWC [B][H*s][W*s][C] float32,
 *   out[b][y*s + i][x*s + j][c] = y[(b*H + y)*W + x][i][j][c] + bias[c]   (an exact copy and one float32 add; bias_or_null == NULL: the copy alone).
 * C a multiple of 4 and y / bias / out 16-byte aligned, else VD3D_E_UNSUPPORTED. */
int vd3d_depth_to_space_bias_nhwc_f32(vd3d_ctx* ctx, const float* y, const float* bias_or_null, int B, int H, int W, int s, int C, float* out);

/* The gather half of a ViT patch embedding (Conv2d(3, C, kernel_size=p, stride=p): kernel == stride, every patch is one GEMM row) for
 * DepthPipe(self_contained=True): x float32 NHWC [B][th][tw][3] (what vd3d_depth_preprocess writes) -> rows float32 [B * gh * gw][Kp], gh = th / p, gw = tw / p
 * (a remainder is dropped, as the convolution drops it), Kp = 3 p^2 rounded up to a multiple of 16 (p = 14: 588 -> 592),
 *   rows[(b * gh + gy) * gw + gx][(c * p + ky) * p + kx] = x[b][gy * p + ky][gx * p + kx][c]   (exact copies, F.unfold's column order);
 * the columns from 3 p^2 on are written as zeros.  vd3d_gemm_x3 on the weight [C][3 p^2] zero-padded to Kp, with the bias, then gives the patch tokens
 * [B][gh * gw][C].  1 <= p <= 64, th, tw >= p, B >= 1, rows 16-byte aligned (x 4-byte), else VD3D_E_UNSUPPORTED and nothing is launched. */
int vd3d_patchify_f32(vd3d_ctx* ctx, const float* x, int B, int th, int tw, int p, float* rows);

/* ---- The BiT ResNet prefix of DPT-Hybrid (MiDaS 3.0; BitEmbeddings + three BitStages of BitBottleneckLayer) under DepthPipe(self_contained=True): its matrix
 * work runs on vd3d_gemm_x3 and the stride-1 tile convolutions; these entry points are everything else.  Activations are float32 NHWC rows [B * H * W][C].
 *
 * The gather half of a k x k convolution run as a GEMM: x [B][H][W][C] -> rows [B * Ho * Wo][Kp], Ho = (H + pad_top + pad_bottom - k) / stride + 1 (Wo alike),
 * Kp = k k C rounded up to a multiple of 16,
 *   rows[(b * Ho + oy) * Wo + ox][(ky * k + kx) * C + c] = x[b][oy * stride - pad_top + ky][ox * stride - pad_left + kx][c], zero outside the map
 * (exact copies: the weight [Cout][C][k][k] permuted to [Cout][k][k][C]); the columns from k k C on are written as zeros.  The four paddings are given apart
 * because TensorFlow's "same" padding is asymmetric (2 / 3 for 7 x 7 stride 2 on an even side, 0 / 1 for 3 x 3 stride 2).  k in {1, 3, 7}, stride 1 | 2, every
 * padding 0 .. k - 1, at least one output pixel, rows 16-byte aligned, x 4-byte (16-byte where C % 4 == 0: 16-byte loads), else VD3D_E_UNSUPPORTED. */
int vd3d_im2col_nhwc_f32(vd3d_ctx* ctx, const float* x, int B, int H, int W, int C, int k, int stride, int pad_top, int pad_bottom, int pad_left, int pad_right,
                         float* rows);

/* 3 x 3 / stride 2 max-pool of x [B][H][W][C] padded by pad_value on the four sides (0 .. 2 each): out [B][Ho][Wo][C], Ho = (H + pad_top + pad_bottom - 3) / 2 + 1.
 * torch.nn.functional.max_pool2d(F.pad(x, ..., value=pad_value), 3, 2): a NaN in a window is that window's result.  C a multiple of 4, x / out 16-byte aligned,
 * at least one output pixel, else VD3D_E_UNSUPPORTED. */
int vd3d_maxpool3x3_s2_nhwc_f32(vd3d_ctx* ctx, const float* x, int B, int H, int W, int C, int pad_top, int pad_bottom, int pad_left, int pad_right,
                                float pad_value, float* out);

/* GroupNorm over x [B][P][C] (P = H W pixels) in G groups of C / G neighbouring channels, with an optional residual and ReLU behind it:
 *   out = [max(., 0)]( (x - mean) * (rstd * gamma[c]) + beta[c] [+ residual] ),  mean and the BIASED variance per (frame, group), rstd = 1 / sqrt(var + eps).
 * Two passes over the data for the statistics -- the mean first, then the sum of (x - mean)^2, never E[x^2] - mean^2 -- and one to apply: three launches, no
 * atomics, every sum in ONE fixed order that depends on (P, C, C / G) alone (csrc/vd3d_bit.hip states it; tests/test_hip_bit_stem.py restates it in NumPy):
 * a frame's result does not depend on its batch and repeats bit for bit.  flags: VD3D_GN_RELU.  out may be x or residual.  workspace: at least
 * vd3d_groupnorm_nhwc_f32_workspace_bytes(B, P, C, G) bytes of device memory (host-only; < 0: shape not built), contents irrelevant.
 * Built: C in {64, 128, 256, 512, 1024} with C / G in {2, 4, 8, 16, 32}; 1 <= B <= 65 535; P <= 2^24; every pointer 16-byte aligned.  Anything else is
 * VD3D_E_UNSUPPORTED and nothing is launched. */
enum { VD3D_GN_RELU = 1 };
int64_t vd3d_groupnorm_nhwc_f32_workspace_bytes(int B, int64_t P, int C, int G);
int vd3d_groupnorm_nhwc_f32(vd3d_ctx* ctx, const float* x, const float* residual_or_null, const float* gamma, const float* beta, float eps, int flags, int B,
                            int64_t P, int C, int G, void* workspace, int64_t workspace_bytes, float* out);

/* ---- DepthPro (transformers' DepthProForDepthEstimation; visiondepth3d_amd/depth_pro.py states both in torch).  "ATen's bilinear" below is
 * F.interpolate(mode="bilinear", align_corners=False, antialias=False) with a size given: equal sizes are the identity; otherwise scale = float(in) / out,
 * src = max(scale (d + 0.5) - 0.5, 0), i0 = min(floor(src), in - 1), l1 = clamp(src - i0, 0, 1), i1 = i0 + (i0 < in - 1), l0 = 1 - l1 and
 * out = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), every operation rounded to float32 on its own.  Every refusal is VD3D_E_UNSUPPORTED with a message,
 * and nothing is launched.
 *
 * DepthProImageProcessor: frames_bgr uint8 [B][H][W][3] -> out float32 planar [B][3][S][S] in R, G, B order.  Rescale and normalise first -- a table of the byte,
 * (float(v) - 255 mean[c]) / (255 std[c]), a subtraction and a division -- then ATen's bilinear of the float image.  mean_host / std_host: 3 floats each, R, G, B.
 * S a multiple of 4, out 16-byte aligned, every side 1 .. 2^20, std non-zero. */
int vd3d_depthpro_preprocess_u8(vd3d_ctx* ctx, const uint8_t* frames_bgr, int B, int H, int W, int S, const float* mean_host, const float* std_host, float* out);
/* DepthProImageProcessor.post_process_depth_estimation: pred float32 [B][S][S] -> out [B][oH][oW] = 1 / clamp(resize(pred * oW / focal), 1e-4, 1e4), with
 * focal = 0.5 oW / tan(0.5 deg2rad(fov[b])) -- fov_or_null: the model's field of view in degrees, float32 [B] in DEVICE memory (no host synchronisation), NULL:
 * no scaling -- resize = ATen's bilinear, skipped for oH == oW == S.  tan is evaluated in float64 and narrowed to float32 (within 1 ulp; the narrowing is a second rounding).  NaN stays NaN. */
int vd3d_depthpro_post_f32(vd3d_ctx* ctx, const float* pred, const float* fov_or_null, int B, int S, int oH, int oW, float* out);
/* The two gathers around DepthPro's three ViT encoders under DepthPipe(encoders=...); visiondepth3d_amd/depth_pro.py states both in NumPy (patches_statement,
 * merge_statement) and the kernels give those values bit for bit.
 *
 * DepthProPatchEncoder's patch pyramid in one launch: pixel_values float32 planar [B][3][S][S] -> patches [(n1^2 + n2^2 + n4^2) B][p][p][3] (pixel-interleaved: the
 * memory vd3d_patchify_f32 reads; the logical tensor is [N][3][p][p]).  Levels in the order full resolution, half, quarter; inside a level patch-major, batch-minor
 * (index l B + b, l the row-major patch position); a level whose image has side s holds (s - p) / stride + 1 patches per side, one where s == p (its stride is then
 * not read).  Half level: 0.25 ((a + b) + (c + d)) over every 2 x 2 cell; quarter level: the same over the 2 x 2 centre of every 4 x 4 cell --
 * F.interpolate(scale_factor=0.5 / 0.25, mode="bilinear") on such sides.  vd3d_depthpro_patches_count (host only): patches per frame, < 0 where a level holds no
 * patch.  S a multiple of 4 up to 2^20, S / 4 >= p >= 1, 4-byte aligned pointers; 16-byte loads and stores where p and the strides in use are multiples of 4 and
 * both pointers 16-byte aligned, 4-byte ones otherwise. */
int64_t vd3d_depthpro_patches_count(int S, int p, int stride_full, int stride_half, int stride_quarter);
int vd3d_depthpro_patches_f32(vd3d_ctx* ctx, const float* pixel_values, int B, int S, int p, int stride_full, int stride_half, int stride_quarter, float* patches);
/* reconstruct_feature_maps in NHWC: rows float32 [n B][T][C] (sequence index l B + b) -> out [B][oh][ow][C].  The leading T - g^2 tokens are dropped; side =
 * int(sqrt(n)) patches per side (1 for n == 1; sequences past side^2 are never read); pad = min(g / 4, padding), 0 for n < 4, trimmed on the edges that meet
 * another patch: merged size M = side g - 2 pad (side - 1); then ATen's bilinear from M x M to oh x ow, skipped (exact copies) for oh == ow == M.  T >= g^2,
 * g <= 4096, sides up to 2^20, 4-byte aligned pointers; 16-byte loads and stores where C is a multiple of 4 and both pointers are 16-byte aligned. */
int vd3d_depthpro_merge_f32(vd3d_ctx* ctx, const float* rows, int n, int B, int T, int C, int g, int padding, int oh, int ow, float* out);

/* ---- ZoeDepth (transformers' ZoeDepthForDepthEstimation; visiondepth3d_amd/zoedepth.py states all four in torch).  Every map is float32 NHWC.  "Bilinear" below is
 * F.interpolate(mode="bilinear", align_corners=True): scale = float(in - 1) / float(out - 1) (0 for out == 1), src = scale d, i0 = min(int(src), in - 1),
 * i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, out = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), every operation rounded to float32 on its own; a
 * zero-weight tap is still multiplied in.  Every refusal (shape, alignment, an output that overlaps an input) is VD3D_E_UNSUPPORTED with a message, and nothing is
 * launched.
 *
 * ZoeDepthImageProcessor: frames_bgr uint8 [B][H][W][3] -> out [B][th][tw][3] in R, G, B order (a channels_last pixel_values tensor).  table_dev: 256 floats in
 * DEVICE memory, the processor's rescale of every byte (the caller builds it with the class's own rescale: float32(float64(v) * (1 / 255)), which is not
 * float32(v) * float32(1 / 255)); then the reflect padding by pad_h / pad_w (np.pad mode="reflect", folded into the gather index), the bilinear resize of the
 * (H + 2 pad_h) x (W + 2 pad_w) image to th x tw, and (v - mean[c]) / std[c] last.  0 <= pad < its side; sides 1 .. 2^20; std non-zero; 4-byte aligned pointers. */
int vd3d_zoedepth_preprocess_u8(vd3d_ctx* ctx, const uint8_t* frames_bgr, const float* table_dev, int B, int H, int W, int pad_h, int pad_w, int th, int tw,
                                const float* mean_host, const float* std_host, float* out);
/* ZoeDepthImageProcessor.post_process_depth_estimation with source_sizes and no target_sizes: pred [B][th][tw] -> out [B][H][W] = the bicubic resize (ATen's:
 * A = -0.75, align_corners=False, no antialias, src = scale (d + 0.5) - 0.5 with scale = float(in) / out, tap indices clamped) of pred to
 * (H + 2 pad_h) x (W + 2 pad_w) with the padding cut off -- evaluated at the surviving rows and columns only.  NaN reaches exactly the pixels that tap it. */
int vd3d_zoedepth_post_f32(vd3d_ctx* ctx, const float* pred, int B, int th, int tw, int H, int W, int pad_h, int pad_w, float* out);
/* ZoeDepthAttractorLayerUnnormed behind its MLP: attractors [B][h][w][nA] (after softplus), prev_bins [B][hp][wp][nb] -> out [B][h][w][nb] =
 * c + (sum_i dx_i / (1 + 300 dx_i dx_i)) [/ nA for mean != 0], c = bilinear(prev_bins), dx_i = a_i - c; the sum runs in ascending i from zero in the module's
 * operation order (dx dx, times 300, plus 1, the division, the accumulation), so the result is the module's float32 loop bit for bit given the same c.
 * nA 1 .. 16; nb a multiple of 4 up to 256; sides up to 2^15; bins 16-byte aligned. */
int vd3d_zoedepth_attractor_f32(vd3d_ctx* ctx, const float* attractors, const float* prev_bins, int B, int h, int w, int hp, int wp, int nA, int nb, int mean, float* out);
/* ZoeDepthConditionalLogBinomialSoftmax and the expectation behind it, per pixel of last [B][H][W][32]: hidden = w1_last [Ch][32] . last (+ wrel [Ch] times the
 * relative-depth plane rel [B][H][W]; both NULL or both given) + bilinear(P [B][hc][wc][Ch]) + b1; exact (erf) GELU; the four outputs w2 [4][Ch] . g + b2; torch's softplus (threshold 20)
 * + 1e-4; p = s0 / (s0 + s1), temperature = (max_temp - min_temp) t0 / (t0 + t1) + min_temp; p and 1 - p clamped to [1e-4, 1]; logits
 * (table[k] + k log p + (nb - 1 - k) log(1 - p)) / temperature; a max-subtracted softmax over the nb bins; out [B][H][W] = its expectation against
 * bilinear(bins [B][hc][wc][nb]).  table: the module's float32 log_binom(nb - 1, k), nb floats.  Every pointer is device memory.  Ch a multiple of 4 up to 128; nb a
 * multiple of 4 up to 256; sides up to 2^15; last, P and bins 16-byte aligned.  The MLP is float32 with fused multiply-adds; softplus, p, the temperature and the
 * logits are evaluated in float64 (a logit reaches (nb - 1) |log 1e-4| and is divided by a temperature as small as min_temp), the exponential of the max-subtracted
 * logit and the two sums in float32. */
int vd3d_zoedepth_bins_f32(vd3d_ctx* ctx, const float* last, const float* rel_or_null, const float* wrel_or_null, const float* P, const float* bins, const float* w1_last,
                           const float* b1, const float* w2, const float* b2, const float* table, double min_temp, double max_temp, int B, int H, int W, int hc, int wc,
                           int Ch, int nb, float* out);

/* ---- preview visualisers: generate_preview_image, core/preview_utils.py:23-84, the exactly defined types.
 * left / right: uint8 BGR [h][w][3] eyes (outputs of vd3d_pixel_shift).  out: [h][w][3], except HSBS: [h][2*(w/2)][3].
 * The colour-mapped heat-maps and the arrow overlay (OpenCV colour-map tables / line rasteriser) return VD3D_E_UNSUPPORTED. */
typedef enum vd3d_preview {
  VD3D_PREVIEW_INTERLACED = 0,   /* even rows left, odd rows right */
  VD3D_PREVIEW_HSBS = 1,         /* cv2.resize(eye, (w/2, h)) (INTER_LINEAR, 11-bit fixed point) + hstack */
  VD3D_PREVIEW_LR_DIFF = 2,      /* cv2.absdiff */
  VD3D_PREVIEW_FEATHER_BLEND = 3,/* the left eye */
  VD3D_PREVIEW_RED_BLUE = 4      /* (right.B, right.G, left.R) */
} vd3d_preview;
int vd3d_preview_image(vd3d_ctx* ctx, int type, const uint8_t* left_bgr, const uint8_t* right_bgr, int h, int w, uint8_t* out_bgr);
/* The colour-mapped types of the same function (core/preview_utils.py:42-66): type 0 "Shift Heatmap" (cv2.normalize NORM_MINMAX),
 * 1 "Shift Heatmap (Abs)", 2 "Shift Heatmap (Clipped +-5px)", 3 "Feather Mask"; shift_map: float32 [h][w] (pixel_shift_cuda's third return),
 * lut_bgr_dev: 256 x 3 uint8 BGR table in device memory -- OpenCV's COLORMAP_JET (types 0-2) / COLORMAP_BONE (3) as the caller obtained it
 * (cv2.applyColorMap(np.arange(256, dtype=np.uint8), cmap)); the library holds no copy of those tables. */
int vd3d_preview_heatmap(vd3d_ctx* ctx, int type, const float* shift_map, int h, int w, const uint8_t* lut_bgr_dev, uint8_t* out_bgr);
/* "Overlay Arrows" (core/preview_utils.py:74-82): the left eye with a green cv2.arrowedLine((x, y) -> (x + int(10 shift), y), tipLength 0.3)
 * at every 20th pixel of every 20th row where |int(10 shift)| > 1.  left_bgr != out_bgr. */
int vd3d_preview_arrows(vd3d_ctx* ctx, const uint8_t* left_bgr, const float* shift_map, int h, int w, uint8_t* out_bgr);

/* ---- stage entry points (the pieces B2 is made of; exported for tests / profiling / sharded runner) */
/* apply_dof_cuda + apply_color_grade + tensor_to_frame + side bars + apply_sharpening + fit + mux
 * (core/render_3d.py:1340-1419) on two u8 eyes. depth_norm is the eye-res normalised depth. */
int vd3d_finish_frame(vd3d_ctx* ctx, const uint8_t* left_bgr, const uint8_t* right_bgr,
                      const float* depth_norm, int eye_h, int eye_w,
                      const vd3d_render_params* p, double focal_depth, int bar_width, int bar_side,
                      uint8_t* out_bgr);
/* exact order statistics on a device plane: torch.quantile semantics (float32 rank, two-branch lerp) */
int vd3d_quantiles(vd3d_ctx* ctx, const float* plane, int64_t n, const float* q_host, int nq, float* out_host);
/* estimate_subject_depth, core/render_3d.py:145-172 (synchronises; test/diagnostic entry) */
int vd3d_subject_depth(vd3d_ctx* ctx, const float* plane, int H, int W, float* out_host);
/* detect_black_bars, core/render_3d.py:293-316, on a device-resident uint8 BGR frame (synchronises; test/diagnostic
 * entry -- vd3d_render_frame runs the same kernel asynchronously when auto_crop_black_bars is set) */
int vd3d_detect_black_bars(vd3d_ctx* ctx, const uint8_t* frame_bgr, int h, int w, int* top_host, int* bottom_host);
/* device-to-device streaming copy used as the measured-peak yardstick for roofline.frac */
int vd3d_stream_copy(vd3d_ctx* ctx, const void* src, void* dst, size_t bytes);
/* The three transcendental operators of the path, elementwise on a device float32 array, with the VALUES torch's CPU kernels give
 * (which is what the reference computes with): op 0 = torch.pow(x, param) for x >= 0 (_signed_pow core/render_3d.py:517, the layer
 * weight :620; SLEEF Sleef_powf_u10 and ATen's special exponents), op 1 = torch.sigmoid(x) (:209; 1 / (1 + Sleef_expf_u10(0 - x))),
 * op 2 = torch.sqrt(x) (:206, :349, :440; MKL VML vsSqrt -- one ULP low on 0.6 % of the inputs).  The kernels of the chain call the
 * same device functions; this entry exists so that they can be compared against the oracle / torch on arbitrary inputs. */
int vd3d_torch_math(vd3d_ctx* ctx, int op, const float* x, float param, float* out, long long n);
/* Ops 0 and 1 of the above as a torch process with `aten_threads` intra-op threads computes them on a contiguous n-element float32 CPU tensor: the SLEEF
 * values, and on the scalar tails of every thread's chunk (vd3d_shift_params::aten_threads) libm's -- (float) pow((double) x, param) with the unrounded
 * Python exponent, 1 / (1 + expf(-x)) with glibc's expf.  aten_threads 0: no tails; < 0: every element takes the tail arithmetic (diagnostic).  The shaping and
 * shift kernels call the same device functions.  n < 2^32. */
int vd3d_torch_math_aten(vd3d_ctx* ctx, int op, const float* x, double param, float* out, long long n, int aten_threads);
/* HIP-event profiling of the stages on the ctx stream ("frame", "ingest", "select_eye", "select_dc", "shape",
 * "select_s1", "warp" (= "shift" + "w1", the fused warp kernel alone), "finish", "handoff", "advance", "pixel_shift", "stream_copy").  vd3d_last_stage_ms = average ms per call since
 * profiling was enabled (-1 if never seen); both getters synchronise. */
int vd3d_set_profiling(vd3d_ctx* ctx, int enable);
/* Route selectors for parity tests and, in development libraries only, launch-policy knobs.  Results NEVER depend on any of them (tested).
 * Product library: which = 3 -- routes of the finishing stage (bit 0: fused kernel in front of a fit it does not take, bit 1: its epilogue as the sharpen / fit /
 * mux kernel behind the unfused DOF kernels; default 3) and which = 4 -- 1: feather_strength <= 0 still runs the mask / window-sum / blend kernels instead of the
 * exact no-feather warp (default 0).  Process-wide plain switches: set them while no frame is in flight.  Every other knob (0 - 2, 5 - 9: tile heights and
 * orders, chain grouping, the parked persistent kernels) returns VD3D_E_UNSUPPORTED unless the library was built with -DVD3D_DEV_KNOBS
 * (bash tools/build_ab.sh dev -DVD3D_DEV_KNOBS); which = -1 queries that (0 = development knobs present).  The VD3D_TUNE environment variable of the Python
 * loader is honoured by development libraries only. */
int vd3d_debug_tune(int which, int value);
float vd3d_last_stage_ms(vd3d_ctx* ctx, const char* stage);
long vd3d_stage_calls(vd3d_ctx* ctx, const char* stage);
/* host-only (works without a GPU): the float32 Gaussian weights the DOF kernels receive for one blur level -- torchvision's _get_gaussian_kernel1d as torch
 * evaluates it on the CPU, incl. torch.sum's summation order (core/render_3d.py:798-806); odd k <= 31.  Tests compare it with torch and the oracle. */
int vd3d_debug_gaussian_kernel1d(int k, float sigma, float* out_host);
/* host-only: the library's restatement of torch.exp on a float32 CPU tensor (oneMKL vsExp, not the rounded exponential) that the DOF weights use */
int vd3d_debug_exp_torch(const float* x_host, float* out_host, long long n);
/* internal planes of the last call (device pointers owned by ctx; tests only).  S: the render / step path without feathering computes the shift values inside the
 * warp kernel and does not write this plane (round 6); vd3d_pixel_shift always does. */
int vd3d_debug_planes(vd3d_ctx* ctx, float** D, float** S, uint8_t** L, uint8_t** R, float** rgb_eye, float** dn_cur);

#ifdef __cplusplus
}
#endif
#endif /* VD3D_H */
