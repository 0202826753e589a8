// vd3d_api.hip -- C ABI of libvd3d_hip.so (include/vd3d.h).  Host-side orchestration only:
// every entry point enqueues kernels on the ctx stream and returns; no host synchronisation
// except where the header says so.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <list>
#include <map>
#include <string>
#include <vector>

#include "vd3d_kernels.h"

#define VD3D_EXPORT extern "C" __attribute__((visibility("default")))

static thread_local char g_err[512] = "";
static int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
#define HIPCHK(x)                                                                                     \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) return set_err(VD3D_E_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

struct vd_prof_rec { std::string name; hipEvent_t a, b; };

struct vd3d_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false, own_stream_escaped = false;
  vd_dev_work* work = nullptr;
  uint32_t* histA = nullptr;  // [VD_NJOBS][VD_NB_A] followed by histB [VD_NJOBS][VD_MAX_T][VD_NB_B]
  uint32_t* histB = nullptr;
  size_t hist_bytes = 0;
  // eye-res planes
  int eye_h = 0, eye_w = 0;
  float* rgb_eye = nullptr; float* tdf = nullptr; float* dn[2] = {nullptr, nullptr};
  int dn_cur = 0;
  // warp-res planes
  int H = 0, W = 0;
  float *dc = nullptr;   // curved depth plane (fused chain)
  float *D = nullptr, *S = nullptr, *e2L = nullptr, *e2R = nullptr, *bL = nullptr, *bR = nullptr;
  float *E2 = nullptr;   // [H][W][2]: gradient mask of both eyes, k_e2w -> W1
  uint8_t *L = nullptr, *R = nullptr, *gL = nullptr, *gR = nullptr;
  uint8_t* gLR = nullptr; size_t gLR_cap = 0;   // [H][2W][3] sharpened eyes side by side (E1 in front of a fit it does not take)
  uint32_t* mm = nullptr; int mm_cap = 0;
  uint32_t* pclip_ws = nullptr; int pclip_cap = 0;    // vd3d_depth_normalize_pclip_u8: [frames][VD_PCLIP_WS_WORDS] radix-select histograms
  vd_lb_ws* lb = nullptr;                             // letterbox tracker state and workspace (vd3d_letterbox.hip), created on first use
  uint32_t* rowflag = nullptr; int rowflag_cap = 0;   // k_autocrop: one flag per source row
  uint8_t* blank_eye = nullptr; size_t blank_cap = 0; // skip_blank_frames: the side-masked source frame (source size)
  // vd3d_render_params::aten_sum_threads > 0: piece plan of the two torch.mean sums (vd3d_atensum.hip) for the current eye size / thread count, and the
  // per-frame piece sums of a batch.  Plans are never overwritten (a queued kernel may still read one): a new key gets new buffers.
  int aten_eh = 0, aten_ew = 0, aten_T = 0, aten_n_small = 0, aten_n_big = 0, aten_nr_crop = 0, aten_nr_mad = 0;
  int* aten_plan = nullptr; float* aten_scratch = nullptr;
  struct vd_aten_entry { int eh, ew, T, n_small, n_big, nr_crop, nr_mad; int* plan; float* scratch; };
  std::vector<vd_aten_entry> aten_cache;   // plans of other (eye size, thread count) keys this context has used (re-used, bounded at 8)
  // the N-thread ATen mode (round 5): planes resized by ATen's premultiplied-weight kernel ahead of W1 (RGB, [3][H][W]) and of the finishing kernels (depth, [H][W])
  float* pm_rgb = nullptr; size_t pm_rgb_cap = 0;
  float* pm_dd = nullptr; size_t pm_dd_cap = 0;
  uint8_t* fmt_eyes = nullptr; size_t fmt_cap = 0;    // vd3d_format_3d_output's own pair of resized VR eyes (never the shared warp-res planes: ADVICE r4)
  bool crop_scalars_dirty = false;                    // fs.crop_top/bottom hold a previous auto-crop result
  // frame sharding (three-phase protocol): per-slot planes of the frames this rank owns inside the current step
  int n_slots = 0, slot_eh = 0, slot_ew = 0, slot_H = 0, slot_W = 0;
  std::vector<float*> slot_rgb, slot_dn, slot_D;
  std::vector<float*> slot_tdf, slot_tdfp;   // measure/replay protocol: filtered plane of the own frame and of the frame before it
  std::vector<const float*> slot_prev;       // where P1 left "the filtered plane of the frame before slot's frame" (slot_tdfp[slot], or the previous slot's slot_tdf inside a batch)
  // batched steps: per frame of a batch (<= VD_MAX_BATCH) its own histogram arena and curved-depth plane, so that the frames' chain
  // kernels run side by side in one launch
  int n_batch = 0; uint32_t* bhist = nullptr; std::vector<float*> bdc;
  float* etab = nullptr;                     // [VD_MAX_STEP + 1][VD_ETAB] replayed normalisation table of the current step
  int* crop_tab = nullptr;                   // [VD_MAX_STEP][4] exchanged auto-crop rectangles of the current step
  bool crop_tab_set = false;
  vd_dev_work* slot_work = nullptr;
  // overlapped pixel passes (vd3d_set_pixel_overlap): vd3d_shard_pixels runs on pix_stream behind the measurement chain of the
  // NEXT step, which stays on `stream`; slot_done[slot] guards the slot's planes against being overwritten too early
  hipStream_t pix_stream = nullptr; bool pix_overlap = false; bool pix_pending = false; bool pix_stream_escaped = false;
  hipEvent_t ev_chain = nullptr, ev_pix_last = nullptr;
  // more than one pixel stream (vd3d_set_pixel_overlap(ctx, n), n = 2 .. VD_MAX_PIX): consecutive pixel passes go round-robin over n
  // streams, each with its own shift plane and warped eyes, so the kernels of neighbouring frames (k_shift / W1 / E1: different LDS, VGPR and
  // latency profiles) share the CUs and the tail of one launch is covered by the next frame's kernels.  Stream 0 = pix_stream with the
  // context's S / L / R.  A pass that needs the context's SHARED fallback planes (unfused warp / finish) first waits for the other
  // streams and is waited for by every later pass (pix_excl_*).
#define VD_MAX_PIX 4
  int n_pix = 1; unsigned pix_rr = 0; int cur_pix = -1; bool cur_excl = false;
  hipStream_t pix_x[VD_MAX_PIX - 1] = {nullptr, nullptr, nullptr}; bool pix_x_escaped[VD_MAX_PIX - 1] = {false, false, false};
  hipEvent_t ev_pix_last_x[VD_MAX_PIX - 1] = {nullptr, nullptr, nullptr}; bool pix_pending_x[VD_MAX_PIX - 1] = {false, false, false};
  float* E2_x[VD_MAX_PIX - 1] = {nullptr, nullptr, nullptr};
  float* S_x[VD_MAX_PIX - 1] = {nullptr, nullptr, nullptr}; uint8_t* L_x[VD_MAX_PIX - 1] = {nullptr, nullptr, nullptr}; uint8_t* R_x[VD_MAX_PIX - 1] = {nullptr, nullptr, nullptr};
  int x_H = 0, x_W = 0;
  hipEvent_t ev_excl = nullptr; bool excl_set = false;
  std::vector<hipEvent_t> slot_done; std::vector<char> slot_busy;
  // dense DOF weight table of the fused finishing kernel (vd_finish_consts::w2) in device memory + the host copy it was uploaded from
  // Tables are never overwritten (a finish kernel of an earlier dof_strength may still be queued on any of the context's streams): every new
  // parameter set gets its own 1.3 KB device table, filled before anything can read it
  struct w2_tab { float host[4][81]; float* dev; };
  std::vector<w2_tab> w2_tabs; int w2_cur = -1;
  // ... and the general table of the unfused dense kernel (k_dof_grade4: any odd tap count up to 31), same never-overwrite rule
  struct wk_tab { int ksz[4]; float kern[4][32]; float* dev; };
  std::vector<wk_tab> wk_tabs; int wk_cur = -1;
  // Pillow-exact front end (vd3d_pilresample.hip): the per-axis coefficient tables of every (input size, output size) this context has met, the
  // normalisation tables of every (mean, std), and the pre-resized frames of vd3d_depth_preprocess_pil.  A table is built once, never overwritten
  // (a queued kernel may read it) and freed with the context; an axis outside the tap budget is remembered with dev == NULL.
  std::list<vd_pil_axis> pil_axes;
  struct pil_lut { float mean[3], stdv[3]; float* dev; };
  std::vector<pil_lut> pil_luts;
  uint8_t* pil_mid = nullptr; size_t pil_mid_cap = 0;
  // profiling
  bool profiling = false;
  std::vector<vd_prof_rec> recs;
  std::vector<hipEvent_t> ev_pool;
  std::map<std::string, std::pair<double, long>> acc;
};

struct StageTimer {
  vd3d_ctx* c; vd_prof_rec r; bool on;
  StageTimer(vd3d_ctx* ctx, const char* name) : c(ctx), on(ctx->profiling) {
    if (!on) return;
    r.name = name;
    auto get = [&]() { hipEvent_t e; if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); } else (void)hipEventCreate(&e); return e; };
    r.a = get(); r.b = get();
    (void)hipEventRecord(r.a, c->stream);
  }
  ~StageTimer() {
    if (!on) return;
    (void)hipEventRecord(r.b, c->stream);
    c->recs.push_back(r);
  }
};

static void prof_collect(vd3d_ctx* c) {
  for (auto& r : c->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      auto& a = c->acc[r.name];
      a.first += ms; a.second += 1;
    }
    c->ev_pool.push_back(r.a); c->ev_pool.push_back(r.b);
  }
  c->recs.clear();
}

// main stream waits until the overlapped pixel pass that still reads `slot` has finished (no-op without overlap)
static int wait_slot(vd3d_ctx* c, int slot) {
  if (c->pix_overlap && slot >= 0 && slot < (int)c->slot_busy.size() && c->slot_busy[slot]) {
    HIPCHK(hipStreamWaitEvent(c->stream, c->slot_done[slot], 0));
    c->slot_busy[slot] = 0;
  }
  return 0;
}
// main stream waits for every outstanding overlapped pixel pass (they share L / R / S and write the caller's outputs)
static int join_pixels(vd3d_ctx* c) {
  bool any = c->pix_pending;
  if (c->pix_pending) {
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_pix_last, 0));
    c->pix_pending = false;
  }
  for (int k = 0; k < VD_MAX_PIX - 1; ++k)
    if (c->pix_pending_x[k]) {
      HIPCHK(hipStreamWaitEvent(c->stream, c->ev_pix_last_x[k], 0));
      c->pix_pending_x[k] = false; any = true;
    }
  if (any) std::fill(c->slot_busy.begin(), c->slot_busy.end(), 0);
  c->excl_set = false;
  return 0;
}
// A pixel pass on one of several pixel streams is about to touch the context's shared fallback planes (e2 / b / graded eyes): order it
// behind the passes already enqueued on the other pixel streams; the caller records ev_excl afterwards, which every later pass waits for.
static int pix_exclusive(vd3d_ctx* c) {
  if (c->cur_pix < 0 || c->n_pix < 2 || c->cur_excl) return 0;
  if (c->cur_pix != 0 && c->pix_pending) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_pix_last, 0));
  for (int k = 0; k < VD_MAX_PIX - 1; ++k)
    if (k + 1 != c->cur_pix && c->pix_pending_x[k]) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_pix_last_x[k], 0));
  c->cur_excl = true;
  return 0;
}

template <class T> static hipError_t re_alloc(T** p, size_t n) {
  if (*p) { hipError_t e = hipFree(*p); *p = nullptr; if (e != hipSuccess) return e; }
  return n ? hipMalloc((void**)p, n * sizeof(T)) : hipSuccess;
}

static int ensure_eye(vd3d_ctx* c, int eh, int ew) {
  if (c->eye_h == eh && c->eye_w == ew) return 0;
  size_t ne = (size_t)eh * ew;
  HIPCHK(re_alloc(&c->rgb_eye, 3 * ne));
  HIPCHK(re_alloc(&c->tdf, ne));
  HIPCHK(re_alloc(&c->dn[0], ne));
  HIPCHK(re_alloc(&c->dn[1], ne));
  if (c->eye_h != 0) {   // the planes were reallocated: TemporalDepthFilter.prev_depth / prev_depth_tensor no longer exist
    const int32_t zero2[2] = {0, 0};
    static_assert(offsetof(vd3d_state, prev_depth_valid) == offsetof(vd3d_state, tdf_valid) + sizeof(int32_t), "adjacent flags");
    HIPCHK(hipMemcpyAsync(&c->work->st.tdf_valid, zero2, sizeof zero2, hipMemcpyHostToDevice, c->stream));
  }
  c->eye_h = eh; c->eye_w = ew; c->dn_cur = 0;
  return 0;
}
static int ensure_work(vd3d_ctx* c, int H, int W) {
  if (c->H == H && c->W == W) return 0;
  size_t n = (size_t)H * W;
  HIPCHK(re_alloc(&c->D, n)); HIPCHK(re_alloc(&c->S, n)); HIPCHK(re_alloc(&c->dc, n));
  HIPCHK(re_alloc(&c->e2L, n)); HIPCHK(re_alloc(&c->e2R, n)); HIPCHK(re_alloc(&c->E2, 2 * n));
  HIPCHK(re_alloc(&c->bL, n)); HIPCHK(re_alloc(&c->bR, n));
  HIPCHK(re_alloc(&c->L, 3 * n)); HIPCHK(re_alloc(&c->R, 3 * n));
  HIPCHK(re_alloc(&c->gL, 3 * n)); HIPCHK(re_alloc(&c->gR, 3 * n));
  c->H = H; c->W = W;
  return 0;
}

// ---------------------------------------------------------------------------------------------
VD3D_EXPORT int vd3d_abi_version(void) { return VD3D_ABI_VERSION; }
VD3D_EXPORT const char* vd3d_last_error(void) { return g_err; }

VD3D_EXPORT void vd3d_shift_params_default(vd3d_shift_params* p) {
  memset(p, 0, sizeof *p);
  p->blur_ksize = 9; p->use_subject_tracking = 1; p->enable_floating_window = 1; p->enable_feathering = 1;
  p->enable_edge_masking = 1; p->enable_dynamic_convergence = 1; p->feather_strength = 10.0;
  p->max_pixel_shift_percent = 0.02; p->parallax_balance = 0.8; p->zero_parallax_strength = 0.0;
  p->convergence_strength = 0.0; p->depth_pop_gamma = 0.85; p->depth_pop_mid = 0.50; p->depth_stretch_lo = 0.05;
  p->depth_stretch_hi = 0.95; p->fg_pop_multiplier = 1.20; p->bg_push_multiplier = 1.10; p->subject_lock_strength = 1.00;
  p->aten_threads = 0; p->reserved0 = 0;
}
VD3D_EXPORT void vd3d_render_params_default(vd3d_render_params* p) {
  memset(p, 0, sizeof *p);
  vd3d_shift_params_default(&p->shift);
  // render_sbs_3d's own keyword defaults (core/render_3d.py:949-984)
  p->shift.feather_strength = 0.0; p->shift.blur_ksize = 1; p->shift.use_subject_tracking = 0; p->shift.enable_floating_window = 0;
  p->ipd_factor = 1.0; p->dof_strength = 0.0; p->sharpness_factor = 0.0;
  p->color_saturation = 1.0; p->color_contrast = 1.0; p->color_brightness = 0.0;
  p->format = VD3D_FMT_HALF_SBS;
  p->dof_dense_conv = 1;   // the reference's convolution order (parity mode) is the default; 0 = separable levels
}

VD3D_EXPORT int vd3d_ctx_create(int device, void* stream, vd3d_ctx** out) {
  if (!out) return set_err(VD3D_E_INVALID, "out is NULL");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return set_err(VD3D_E_INVALID, "device %d out of range (%d visible)", device, ndev);
  HIPCHK(hipSetDevice(device));
  vd3d_ctx* c = new vd3d_ctx();
  c->device = device;
  if (stream == VD3D_STREAM_PRIVATE) { HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
  else c->stream = (hipStream_t)stream;  // NULL = the default stream
  HIPCHK(hipMalloc((void**)&c->work, sizeof(vd_dev_work)));
  HIPCHK(hipMemsetAsync(c->work, 0, sizeof(vd_dev_work), c->stream));
  const size_t nA = (size_t)VD_NJOBS * VD_NB_A, nB = (size_t)VD_NJOBS * VD_MAX_T * (VD_NB_B + VD_NB_BC);
  c->hist_bytes = (nA + nB) * sizeof(uint32_t);
  HIPCHK(hipMalloc((void**)&c->histA, c->hist_bytes));
  c->histB = c->histA + nA;
  *out = c;
  return 0;
}
VD3D_EXPORT int vd3d_ctx_destroy(vd3d_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  prof_collect(c);
  for (auto e : c->ev_pool) (void)hipEventDestroy(e);
  void* ptrs[] = {c->work, c->histA, c->rgb_eye, c->tdf, c->dn[0], c->dn[1], c->D, c->S, c->e2L, c->e2R, c->E2, c->bL, c->bR, c->L, c->R, c->gL, c->gR, c->gLR, c->mm, c->dc, c->rowflag, c->etab, c->crop_tab, c->blank_eye, c->fmt_eyes, c->aten_plan, c->aten_scratch, c->pm_rgb, c->pm_dd, c->pclip_ws};
  for (const auto& e : c->aten_cache) { (void)hipFree(e.plan); (void)hipFree(e.scratch); }
  for (auto& t : c->w2_tabs) (void)hipFree(t.dev);
  for (auto& t : c->wk_tabs) (void)hipFree(t.dev);
  for (auto& a : c->pil_axes) if (a.dev) (void)hipFree(a.dev);
  for (auto& t : c->pil_luts) (void)hipFree(t.dev);
  if (c->pil_mid) (void)hipFree(c->pil_mid);
  for (void* p : ptrs) if (p) (void)hipFree(p);
  vd_lb_free(c->lb);
  for (auto* v : {&c->slot_rgb, &c->slot_dn, &c->slot_D, &c->slot_tdf, &c->slot_tdfp})
    for (float* q : *v) (void)hipFree(q);
  if (c->slot_work) (void)hipFree(c->slot_work);
  for (float* q : c->bdc) (void)hipFree(q);
  if (c->bhist) (void)hipFree(c->bhist);
  for (int k = 0; k < VD_MAX_PIX - 1; ++k) {
    if (c->pix_x[k]) { (void)hipStreamSynchronize(c->pix_x[k]); if (!c->pix_x_escaped[k]) (void)hipStreamDestroy(c->pix_x[k]); }
    if (c->ev_pix_last_x[k]) (void)hipEventDestroy(c->ev_pix_last_x[k]);
    if (c->S_x[k]) (void)hipFree(c->S_x[k]);
    if (c->E2_x[k]) (void)hipFree(c->E2_x[k]);
    if (c->L_x[k]) (void)hipFree(c->L_x[k]);
    if (c->R_x[k]) (void)hipFree(c->R_x[k]);
  }
  if (c->ev_excl) (void)hipEventDestroy(c->ev_excl);
  if (c->pix_stream) { (void)hipStreamSynchronize(c->pix_stream); if (!c->pix_stream_escaped) (void)hipStreamDestroy(c->pix_stream); }
  for (auto e : c->slot_done) (void)hipEventDestroy(e);
  if (c->ev_chain) (void)hipEventDestroy(c->ev_chain);
  if (c->ev_pix_last) (void)hipEventDestroy(c->ev_pix_last);
  if (c->own_stream && !c->own_stream_escaped) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}
VD3D_EXPORT int vd3d_sync(vd3d_ctx* c) {
  if (c->pix_stream) HIPCHK(hipStreamSynchronize(c->pix_stream));
  for (int k = 0; k < VD_MAX_PIX - 1; ++k) if (c->pix_x[k]) HIPCHK(hipStreamSynchronize(c->pix_x[k]));
  HIPCHK(hipStreamSynchronize(c->stream));
  prof_collect(c);
  return 0;
}
VD3D_EXPORT void* vd3d_ctx_stream(vd3d_ctx* c) {
  if (c && c->own_stream) c->own_stream_escaped = true;   // see vd3d_ctx_pixel_stream
  return c ? (void*)c->stream : nullptr;
}
// Re-target a context that enqueues on a caller-owned stream (e.g. whatever stream is current in PyTorch at call time).  Work already
// enqueued stays on the old stream; the new stream is ordered behind it with an event, so the context's planes are never raced.
VD3D_EXPORT int vd3d_ctx_set_stream(vd3d_ctx* c, void* stream) {
  if (!c) return set_err(VD3D_E_INVALID, "NULL context");
  if (c->own_stream) return set_err(VD3D_E_INVALID, "the context owns a private stream (VD3D_STREAM_PRIVATE)");
  if ((hipStream_t)stream == c->stream) return 0;
  HIPCHK(hipSetDevice(c->device));
  int rc = join_pixels(c);
  if (rc) return rc;
  hipEvent_t e;
  HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipEventRecord(e, c->stream));
  HIPCHK(hipStreamWaitEvent((hipStream_t)stream, e, 0));
  HIPCHK(hipEventDestroy(e));
  c->stream = (hipStream_t)stream;
  return 0;
}
// The handle escapes to the caller (PyTorch wraps it and may record events on it when tensors marked with record_stream() are freed, possibly
// after the context is gone): from then on the stream is never destroyed (vd3d_ctx_destroy leaves it to the process).
VD3D_EXPORT void* vd3d_ctx_pixel_stream(vd3d_ctx* c) {
  if (!c) return nullptr;
  if (c->pix_stream) c->pix_stream_escaped = true;
  return (void*)c->pix_stream;
}
// pixel stream k of vd3d_set_pixel_overlap(ctx, n) (k = 0: vd3d_ctx_pixel_stream); NULL beyond the streams created so far
VD3D_EXPORT void* vd3d_ctx_pixel_stream_k(vd3d_ctx* c, int k) {
  if (!c || k < 0 || k >= VD_MAX_PIX) return nullptr;
  if (k == 0) return vd3d_ctx_pixel_stream(c);
  if (c->pix_x[k - 1]) c->pix_x_escaped[k - 1] = true;
  return (void*)c->pix_x[k - 1];
}

// ---- state ------------------------------------------------------------------------------------
VD3D_EXPORT int vd3d_state_export(vd3d_ctx* c, vd3d_state* out) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out, &c->work->st, sizeof(vd3d_state), hipMemcpyDeviceToHost, c->stream));
  return vd3d_sync(c);
}
VD3D_EXPORT int vd3d_state_import(vd3d_ctx* c, const vd3d_state* in) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(&c->work->st, in, sizeof(vd3d_state), hipMemcpyHostToDevice, c->stream));
  return vd3d_sync(c);
}
VD3D_EXPORT int vd3d_state_reset(vd3d_ctx* c) {
  vd3d_state z;
  memset(&z, 0, sizeof z);
  return vd3d_state_import(c, &z);
}
VD3D_EXPORT int vd3d_state_new_clip(vd3d_ctx* c) {  // what render_sbs_3d re-creates per call (:1174-1182)
  vd3d_state s;
  int rc = vd3d_state_export(c, &s);
  if (rc) return rc;
  s.smooth_valid = 0; s.tdf_valid = 0; s.prev_depth_valid = 0; s.focal_valid = 0;
  return vd3d_state_import(c, &s);
}
VD3D_EXPORT int vd3d_state_planes(vd3d_ctx* c, float** tdf_prev, float** norm_prev, int* eye_h, int* eye_w) {
  if (tdf_prev) *tdf_prev = c->tdf;
  if (norm_prev) *norm_prev = c->dn[c->dn_cur ^ 1];  // the plane the NEXT frame treats as d_{t-1}
  if (eye_h) *eye_h = c->eye_h;
  if (eye_w) *eye_w = c->eye_w;
  return 0;
}
VD3D_EXPORT int vd3d_last_scalars(vd3d_ctx* c, vd3d_frame_scalars* out) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out, &c->work->fs, sizeof(vd3d_frame_scalars), hipMemcpyDeviceToHost, c->stream));
  return vd3d_sync(c);
}

// the current plan goes back into the context's cache / a cached plan becomes current
static void aten_cache_put(vd3d_ctx* c) {
  if (!c->aten_plan) return;
  c->aten_cache.push_back(vd3d_ctx::vd_aten_entry{c->aten_eh, c->aten_ew, c->aten_T, c->aten_n_small, c->aten_n_big, c->aten_nr_crop, c->aten_nr_mad, c->aten_plan, c->aten_scratch});
  c->aten_plan = nullptr; c->aten_scratch = nullptr; c->aten_eh = c->aten_ew = c->aten_T = -1;
}
static bool aten_cache_get(vd3d_ctx* c, int eh, int ew, int T) {
  for (size_t i = 0; i < c->aten_cache.size(); ++i) {
    const vd3d_ctx::vd_aten_entry e = c->aten_cache[i];
    if (e.eh != eh || e.ew != ew || e.T != T) continue;
    c->aten_cache.erase(c->aten_cache.begin() + (long)i);
    c->aten_eh = eh; c->aten_ew = ew; c->aten_T = T;
    c->aten_n_small = e.n_small; c->aten_n_big = e.n_big; c->aten_nr_crop = e.nr_crop; c->aten_nr_mad = e.nr_mad;
    c->aten_plan = e.plan; c->aten_scratch = e.scratch;
    return true;
  }
  return false;
}

// vd3d_render_params::aten_sum_threads > 0: the two torch.mean calls of the loop body in ATen's float32 summation order (vd3d_atensum.hip)
static int aten_setup(vd3d_ctx* c, const vd3d_render_params* p, vd_stage_args* a) {
  a->aten_threads = 0;
  const int T = p->aten_sum_threads;
  if (T <= 0) return 0;
  if (c->aten_eh != p->eye_h || c->aten_ew != p->eye_w || c->aten_T != T) {
    // a small per-key cache: a context that alternates between eye sizes / thread counts re-uses its plans instead of allocating a new pair
    // per change; a replaced key's buffers stay valid (queued launches may still read them) and are handed back out when the key returns
    aten_cache_put(c);
    if (!aten_cache_get(c, p->eye_h, p->eye_w, T)) {
      std::vector<int> flat;
      int ns = 0, nb = 0, nrc = 0, nrm = 0;
      if (!vd_aten_plan_build(p->eye_h, p->eye_w, T, flat, &ns, &nb, &nrc, &nrm))
        return set_err(VD3D_E_UNSUPPORTED, "aten_sum_threads %d with %dx%d eyes: outside the restated range (1 .. 1024 threads)", T, p->eye_w, p->eye_h);
      if (c->aten_cache.size() >= 8) {   // bounded: drain the stream once, then free the oldest entry
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->pix_stream) HIPCHK(hipStreamSynchronize(c->pix_stream));
        for (int k = 0; k < VD_MAX_PIX - 1; ++k) if (c->pix_x[k]) HIPCHK(hipStreamSynchronize(c->pix_x[k]));
        (void)hipFree(c->aten_cache.front().plan); (void)hipFree(c->aten_cache.front().scratch);
        c->aten_cache.erase(c->aten_cache.begin());
      }
      c->aten_plan = nullptr; c->aten_scratch = nullptr;
      HIPCHK(hipMalloc((void**)&c->aten_plan, flat.size() * sizeof(int)));
      HIPCHK(hipMemcpy(c->aten_plan, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));   // a fresh buffer: nothing queued reads it yet
      HIPCHK(hipMalloc((void**)&c->aten_scratch, (size_t)VD_MAX_BATCH * (size_t)(ns + nb) * sizeof(float)));
      c->aten_eh = p->eye_h; c->aten_ew = p->eye_w; c->aten_T = T;
      c->aten_n_small = ns; c->aten_n_big = nb; c->aten_nr_crop = nrc; c->aten_nr_mad = nrm;
    }
  }
  a->aten_threads = T; a->aten_n_small = c->aten_n_small; a->aten_n_big = c->aten_n_big; a->aten_nr_crop = c->aten_nr_crop; a->aten_nr_mad = c->aten_nr_mad;
  a->aten_plan = c->aten_plan; a->aten_scratch = c->aten_scratch;
  return 0;
}

// ---- shared middle section: shaped depth, s1, shift, feather, warp --------------------------------
static int check_shift_params(const vd3d_shift_params* p, int H, int W) {
  if (W < 2 || H < 2) return set_err(VD3D_E_INVALID, "warp size %dx%d too small", W, H);
  if ((long long)H * W >= (1ll << 31)) return set_err(VD3D_E_INVALID, "warp size too large");
  if (p->blur_ksize < 1) return set_err(VD3D_E_INVALID, "blur_ksize must be >= 1 (avg_pool2d raises)");
  if (p->blur_ksize > PL_KMAX_HOST) return set_err(VD3D_E_UNSUPPORTED, "blur_ksize %d > %d not built", p->blur_ksize, PL_KMAX_HOST);
  return 0;
}

// The shift parameters as the WARP stage sees them.  feather_shift_edges (core/render_3d.py:328-374) with feather_strength <= 0 is an exact no-op:
// edge_mask = clamp(grad * fs, 0, 1) = 0 everywhere (the gradient magnitude is a finite non-negative number), its k x k average is 0, and
// shifted * (1 - 0) + original * 0 = shifted (the samples are non-negative, so no signed zero survives; the final clamp(0, 1) only touches values the
// uint8 conversion of tensor_to_frame maps to the same byte) -- so the mask kernel (k_e2w), the window sums and the blend are not run at all.  This is
// the GUI's own default configuration (VisionDepth3D.py:1405-1453: feather_strength 0.0, blur_ksize 1).  k_shift keeps the caller's feather_strength:
// suppress_artifacts_with_edge_mask uses it on its own (:204-216).  vd3d_debug_tune(4, 1) keeps the long way (A/B, tests).
static int g_feather0_long = 0;
static vd3d_shift_params warp_stage_params(const vd3d_shift_params& sp) {
  vd3d_shift_params w = sp;
  if (w.enable_feathering && w.feather_strength <= 0.0 && !g_feather0_long) w.enable_feathering = 0;
  return w;
}

// the context's own planes and control block as a batch of one frame (sequential entry points)
static vd_batch batch_of_one(vd3d_ctx* c) {
  vd_batch b;
  memset(&b, 0, sizeof b);
  b.n = 1; b.w_main = c->work;
  vd_batch_frame& F = b.f[0];
  F.w = c->work; F.histA = c->histA; F.histB = c->histB;
  F.rgb_eye = c->rgb_eye; F.tdf = c->tdf; F.tdf_prev = c->tdf;   // the plane EMA updates c->tdf in place
  F.dc = c->dc; F.D = c->D;
  return b;
}

// N-thread ATen mode: a resize ATen runs with its premultiplied-weight kernel (vd_interp_premult) is done here, into a scratch plane of the context, and the
// consumer (W1, the finishing kernels) is then called with identity geometry.  The scratch is shared by the context's pixel streams: callers on one of them go through
// pix_exclusive first.
static int premult_resize(vd3d_ctx* c, int C, const float** plane, int* ih, int* iw, int H, int W, int aten_threads, float** scratch, size_t* cap) {
  if ((*ih == H && *iw == W) || !vd_interp_premult(C, H, W, aten_threads)) return 0;
  const size_t need = (size_t)C * H * W;
  if (*cap < need) { HIPCHK(hipDeviceSynchronize()); HIPCHK(re_alloc(scratch, need)); *cap = need; }
  vd_launch_interp_planes(c->stream, *plane, C, *ih, *iw, *scratch, H, W, 1);
  *plane = *scratch; *ih = H; *iw = W;
  return 0;
}

static int run_shift_and_warp(vd3d_ctx* c, const float* rgb, const float* depth_plane, int ih, int iw, int W, int H,
                              const vd3d_shift_params& sp, vd_stage_args a, bool skip_pixels = false) {
  hipStream_t s = c->stream;
  {
    StageTimer t(c, "select_dc");   // fused chain: norm + stage1 (A1), b1 (B1), shape (+A2), b2 (B2)
    vd_batch b = batch_of_one(c);   // render path: depth_plane = dn_cur (written by K3a from c->tdf); bare pixel_shift_cuda: the caller's plane
    b.f[0].dn = const_cast<float*>(depth_plane);
    b.f[0].dn_prev = a.have_eye ? c->dn[c->dn_cur ^ 1] : nullptr;
    vd_launch_chain_work(s, b, a.have_eye, ih, iw, H, W, (float)sp.depth_pop_mid, (float)sp.depth_pop_gamma, a);
  }
  if (!skip_pixels) { StageTimer t(c, "warp");
    { int rcp = premult_resize(c, 3, &rgb, &ih, &iw, H, W, sp.aten_threads, &c->pm_rgb, &c->pm_rgb_cap); if (rcp) return rcp; }
    const vd3d_shift_params spw = warp_stage_params(sp);   // feather_strength <= 0: the exact no-feather kernels
    const bool pre = spw.enable_feathering && vd_warp_fused_ok(ih, iw, H, W, spw);   // k_e2w -> W1 (see shard_pixels_impl)
    // without feathering W1 computes the shift values of its own tile (round 6); this entry point keeps the plane (its callers can ask for it)
    const bool fold = vd_warp_fold_ok(ih, iw, H, W, spw, sp);
    const vd_shift_fold ff = {c->work, sp, c->S};
    if (!fold) { StageTimer t1(c, "shift"); vd_launch_shift(s, c->D, H, W, c->work, sp, c->S); }
    bool fused = false;
    { StageTimer t2(c, "w1");
      if (pre) { StageTimer t3(c, "e2w"); vd_launch_e2w(s, c->D, c->S, H, W, (float)spw.feather_strength, c->E2); }
      fused = vd_launch_warp_fused(s, rgb, ih, iw, c->D, c->S, H, W, spw, c->L, c->R, pre ? c->E2 : nullptr, fold ? &ff : nullptr); }
    if (!fused && fold) { StageTimer t1(c, "shift"); vd_launch_shift(s, c->D, H, W, c->work, sp, c->S); }
    if (!fused) {   // blur sizes / frame sizes the fused kernel refuses (its LDS tile would not fit): one stage per kernel
    if (spw.enable_feathering) {
      vd_launch_e2(s, c->D, c->S, H, W, (float)spw.feather_strength, c->e2L, c->e2R);
      vd_launch_pool(s, c->e2L, c->e2R, H, W, spw.blur_ksize, c->bL, c->bR);
    }
    vd_launch_warp(s, rgb, ih, iw, c->S, c->bL, c->bR, H, W, spw.enable_feathering ? 1 : 0, c->L, c->R);
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_pixel_shift(vd3d_ctx* c, const float* rgb_chw, const float* depth, int in_h, int in_w, int W, int H,
                                 const vd3d_shift_params* p, uint8_t* left_bgr, uint8_t* right_bgr, float* shift_or_null) {
  if (!c || !rgb_chw || !depth || !p || !left_bgr || !right_bgr) return set_err(VD3D_E_INVALID, "NULL argument");
  if (in_h < 1 || in_w < 1) return set_err(VD3D_E_INVALID, "bad input size");
  int rc = check_shift_params(p, H, W);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = join_pixels(c))) return rc;
  if ((rc = ensure_work(c, H, W))) return rc;
  StageTimer tf(c, "pixel_shift");
  HIPCHK(hipMemsetAsync(c->histA, 0, c->hist_bytes, c->stream));
  vd_stage_args a;
  memset(&a, 0, sizeof a);
  a.have_eye = 0; a.W = W; a.H = H; a.shift = *p; a.ipd_factor = 0.0;
  rc = run_shift_and_warp(c, rgb_chw, depth, in_h, in_w, W, H, *p, a);
  if (rc) return rc;
  const size_t n = (size_t)H * W;
  HIPCHK(hipMemcpyAsync(left_bgr, c->L, 3 * n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(right_bgr, c->R, 3 * n, hipMemcpyDeviceToDevice, c->stream));
  if (shift_or_null) HIPCHK(hipMemcpyAsync(shift_or_null, c->S, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// ---- finishing constants ------------------------------------------------------------------------
static float linspace_host(float start, float end, int steps, int i) {
  if (steps == 1) return start;
  float step = (end - start) / (float)(steps - 1);
  if (i < steps / 2) return fmaf(step, (float)i, start);
  return fmaf(-step, (float)(steps - 1 - i), end);
}
// torch.sum of a contiguous float32 vector in ATen's CPU order (256-bit reduction kernels: 8 lanes, four interleaved vector accumulators, the n % 8 tail
// first, then the lanes in order; below 8 elements four interleaved scalar accumulators; n < 512) -- what `pdf.sum()` of torchvision's _get_gaussian_kernel1d evaluates to.  Same rule as the oracle's sum_aten_f32
// (written independently there); tests/test_aten_restatements.py pins both against torch.sum and against each other through vd3d_debug_gaussian_kernel1d.
static float host_sum_aten(const float* v, int n) {
  if (n < 8) {   // no full vector: the scalar variant (four interleaved scalar accumulators, leftovers into the first)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) { s0 += v[i]; s1 += v[i + 1]; s2 += v[i + 2]; s3 += v[i + 3]; }
    for (; i < n; ++i) s0 += v[i];
    return ((s0 + s1) + s2) + s3;
  }
  const int nv = n >> 3, nq = nv >> 2;
  float acc[4][8];
  for (int j = 0; j < 4; ++j)
    for (int l = 0; l < 8; ++l) acc[j][l] = 0.f;
  for (int i = 0; i < nv; ++i) {
    float* a = acc[i < 4 * nq ? (i & 3) : 0];
    for (int l = 0; l < 8; ++l) a[l] += v[8 * i + l];
  }
  for (int l = 0; l < 8; ++l) acc[0][l] = ((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l];
  float fin = 0.f;
  for (int i = 8 * nv; i < n; ++i) fin += v[i];
  for (int l = 0; l < 8; ++l) fin += acc[0][l];
  return fin;
}
// torch.exp of a float32 on the CPU = oneMKL VML vsExp (high accuracy, AVX-512 path): a table-driven float32 routine, NOT the rounded
// exponential (1.4 % of the inputs of [-8, 0] are an ULP off).  Host-side restatement for the DOF weights (the oracle holds an independent one
// with literal tables; tests/test_aten_restatements.py compares both with torch on every blur level): 2^(j/32) as a float32 head and a
// relative float32 tail, both derived here from their definitions in extended precision; range reduction t = floor(32 x log2 e) / 32 (the
// library's fused multiply-add rounds toward zero onto a positive shifter), r = x - t ln 2 in two fused steps, a degree-3 polynomial tail.
static float host_exp_torch(float x) {
  if (!(fabsf(x) < 87.0f)) return (float)exp((double)x);   // the library's special-case path is not restated (never reached: x in [-8.5, 0])
  struct exp_tabs {   // function-local static of class type: C++11 initialises it once, thread-safely (one context per thread is a supported pattern)
    float th[32], tl[32];
    exp_tabs() {
      for (int j = 0; j < 32; ++j) {
        const long double v = exp2l((long double)j / 32.0L);
        th[j] = (float)v;
        tl[j] = (float)((v - (long double)th[j]) / (long double)th[j]);
      }
    }
  };
  static const exp_tabs tabs;
  const float* th = tabs.th; const float* tl = tabs.tl;
  union { uint32_t u; float f; } c;
  c.u = 0x3fb8aa3bu; const float l2e = c.f;            // log2(e) as the library rounds it
  c.u = 0x3f317218u; const float ln2_hi = c.f;         // ln 2 = ln2_hi - 1.9046542e-09
  c.u = 0x3e2aabf3u; const float c3 = c.f;
  c.u = 0x3f0000f6u; const float c2 = c.f;
  const double t = floor((double)x * (double)l2e * 32.0) * (1.0 / 32.0);
  const long long m32 = (long long)floor((double)x * (double)l2e * 32.0);
  const int j = (int)(m32 & 31);                        // two's complement: the non-negative residue
  const float n = (float)t;
  float r = fmaf(n, -ln2_hi, x);
  r = fmaf(n, 1.9046542e-09f, r);
  const float q = fmaf(fmaf(r, c3, c2), r * r, tl[j] + r);
  const float sc = ldexpf(th[j], (int)floor(t));
  return fmaf(q, sc, sc);
}
// torchvision _get_gaussian_kernel1d in float32 (core/render_3d.py:798-806): k <= 2 DF_RMAX_HOST + 1 taps into out
static void host_gaussian_kernel1d(int k, float sigma, float* out) {
  const float half = (float)((k - 1) * 0.5);
  for (int i = 0; i < k; ++i) {
    float x = linspace_host(-half, half, k, i);
    float t = x / sigma;
    out[i] = host_exp_torch(-0.5f * (t * t));
  }
  const float sum = host_sum_aten(out, k);
  for (int i = 0; i < k; ++i) out[i] = out[i] / sum;
}
// host-only: the product's restatement of torch.exp (MKL vsExp) on n floats -- compared with torch and with the oracle's on the CPU
VD3D_EXPORT int vd3d_debug_exp_torch(const float* x_host, float* out_host, long long n) {
  if (n < 0 || (n > 0 && (!x_host || !out_host))) return set_err(VD3D_E_INVALID, "vd3d_debug_exp_torch: host pointers");
  for (long long i = 0; i < n; ++i) out_host[i] = host_exp_torch(x_host[i]);
  return 0;
}
VD3D_EXPORT int vd3d_debug_gaussian_kernel1d(int k, float sigma, float* out_host) {   // host-only (no GPU needed): the weights the DOF kernels are given
  if (k < 1 || k > 2 * DF_RMAX_HOST + 1 || !(k & 1) || !out_host || !(sigma > 0.f)) return set_err(VD3D_E_INVALID, "gaussian_kernel1d: odd k <= %d, sigma > 0", 2 * DF_RMAX_HOST + 1);
  host_gaussian_kernel1d(k, sigma, out_host);
  return 0;
}

static int make_finish_consts(const vd3d_render_params* p, vd_finish_consts* fc) {
  memset(fc, 0, sizeof *fc);
  const int NL = 5;
  if (p->dof_strength > 0.0) {
    fc->nlev = NL - 1;
    for (int l = 1; l < NL; ++l) {  // apply_dof_cuda :798-806 + torchvision _get_gaussian_kernel1d
      float sigma = linspace_host(0.f, (float)p->dof_strength, NL, l);
      int k = (int)(2 * ceil(2 * (double)sigma) + 1);
      if (k > 2 * DF_RMAX_HOST + 1) return set_err(VD3D_E_UNSUPPORTED, "dof_strength %.3f needs a %d-tap Gaussian (> %d)", p->dof_strength, k, 2 * DF_RMAX_HOST + 1);
      fc->ksz[l - 1] = k;
      host_gaussian_kernel1d(k, sigma, fc->kern[l - 1]);
      if (k <= 9)   // dense association: weight of tap (i, j) = the float32 product of the two 1-D weights (what torchvision's outer product holds)
        for (int i = 0; i < k; ++i)
          for (int j = 0; j < k; ++j) fc->w2[l - 1][i * k + j] = fc->kern[l - 1][i] * fc->kern[l - 1][j];
    }
  }
  fc->fw = (float)(0.35 + 1e-6);
  fc->imax = (float)((NL - 1) - 1e-6);
  fc->sat = (float)p->color_saturation; fc->con = (float)p->color_contrast; fc->bri = (float)p->color_brightness;
  // apply_sharpening :719-728: float32 kernel / np.sum (numpy pairwise order for 9 elements)
  const float c0 = (float)(5.0 + p->sharpness_factor);
  float ks = ((0.f + -1.f) + (0.f + -1.f)) + ((c0 + -1.f) + (0.f + -1.f));
  ks = ks + 0.f;
  fc->sharp_kn = ks != 0.f ? -1.f / ks : -1.f;
  fc->sharp_kc = ks != 0.f ? c0 / ks : c0;
  return 0;
}

#define VD_AREA_MAXT_HOST 12
static int check_fit(const vd3d_render_params* p) {
  // VR: format_3d_output's cv2.resize(eye,(1440,1600)) is the identity only for the 1440x1600 eyes render_sbs_3d makes (:1104,1127)
  if (p->format == VD3D_FMT_VR && (p->fit_w != 1440 || p->fit_h != 1600))
    return set_err(VD3D_E_UNSUPPORTED, "VR with a %dx%d eye canvas would need format_3d_output's INTER_LINEAR resize (not built)", p->fit_w, p->fit_h);
  if (p->format < 0 || p->format > VD3D_FMT_INTERLACED) return set_err(VD3D_E_INVALID, "unknown format %d", p->format);
  int in_w, in_h;
  if (p->format == VD3D_FMT_HALF_SBS) { in_w = p->fit_w; in_h = p->fit_h; }
  else {
    const double ta = (double)p->fit_w / p->fit_h, ca = (double)p->warp_w / p->warp_h;
    if (ca > ta) { in_w = p->fit_w; in_h = (int)(p->fit_w / ca); }
    else { in_h = p->fit_h; in_w = (int)(ca * p->fit_h); }
  }
  if (in_w < 1 || in_h < 1) return set_err(VD3D_E_INVALID, "empty fit %dx%d", in_w, in_h);
  const bool upscale = in_w > p->warp_w || in_h > p->warp_h;   // OpenCV: linear machinery with area-mode coefficients (k_sharp_mux)
  if (!upscale && (p->warp_w % in_w || p->warp_h % in_h) && ((double)p->warp_w / in_w > VD_AREA_MAXT_HOST - 2 || (double)p->warp_h / in_h > VD_AREA_MAXT_HOST - 2))
    return set_err(VD3D_E_UNSUPPORTED, "fractional INTER_AREA ratio above %d not built", VD_AREA_MAXT_HOST - 2);
  const int mux_w = (p->format == VD3D_FMT_HALF_SBS || p->format == VD3D_FMT_FULL_SBS || p->format == VD3D_FMT_VR) ? 2 * p->fit_w : p->fit_w;
  if (p->out_w != mux_w || p->out_h != p->fit_h) return set_err(VD3D_E_INVALID, "out size %dx%d does not match mux %dx%d", p->out_w, p->out_h, mux_w, p->fit_h);
  return 0;
}

static int g_fused_fit = getenv("VD3D_FUSED_FIT") ? atoi(getenv("VD3D_FUSED_FIT")) : 3;   // bit 0: E1 in front of a fit it does not take; bit 1: k_sharp_fit behind k_dof_grade4.  VD3D_FUSED_FIT=0 / vd3d_debug_tune(3, 0): the unfused DOF / grade kernels in front of every fit E1 does not take (A/B, tests)
static int run_finish(vd3d_ctx* c, const uint8_t* L, const uint8_t* R, const float* dn, int eh, int ew,
                      const vd3d_render_params* p, const vd_finish_consts& fc, float focal, int use_override, int bw, int bs,
                      uint8_t* out, const vd_dev_work* wk = nullptr) {
  StageTimer t(c, "finish");
  if (!wk) wk = c->work;
  if (fc.nlev && !(eh == p->warp_h && ew == p->warp_w) && vd_interp_premult(1, p->warp_h, p->warp_w, p->aten_sum_threads)) {   // depth_for_dof (:1347-1350) by ATen's other kernel
    int rcx = pix_exclusive(c); if (rcx) return rcx;
    if ((rcx = premult_resize(c, 1, &dn, &eh, &ew, p->warp_h, p->warp_w, p->aten_sum_threads, &c->pm_dd, &c->pm_dd_cap))) return rcx;
  }
  const int dense = (p->dof_dense_conv && fc.nlev) ? 1 : 0;   // the reference's dense k x k conv order
  const float* d_w2 = nullptr;
  if (dense) {
    if (c->w2_cur < 0 || memcmp(c->w2_tabs[c->w2_cur].host, fc.w2, sizeof fc.w2) != 0) {   // first frame or a new dof_strength (rare)
      c->w2_cur = -1;
      for (size_t i = 0; i < c->w2_tabs.size(); ++i)
        if (memcmp(c->w2_tabs[i].host, fc.w2, sizeof fc.w2) == 0) c->w2_cur = (int)i;
      if (c->w2_cur < 0) {
        if (c->w2_tabs.size() >= 64) {   // a caller sweeping the slider: drain every stream of the context once, then recycle all tables
          HIPCHK(hipDeviceSynchronize());
          for (auto& t : c->w2_tabs) (void)hipFree(t.dev);
          c->w2_tabs.clear();
        }
        vd3d_ctx::w2_tab t;
        memcpy(t.host, fc.w2, sizeof fc.w2);
        HIPCHK(hipMalloc((void**)&t.dev, sizeof fc.w2));
        HIPCHK(hipMemcpy(t.dev, t.host, sizeof fc.w2, hipMemcpyHostToDevice));   // a fresh buffer: nothing queued reads it yet
        c->w2_tabs.push_back(t);
        c->w2_cur = (int)c->w2_tabs.size() - 1;
      }
    }
    d_w2 = c->w2_tabs[c->w2_cur].dev;
  }
  if (vd_launch_finish_fused(c->stream, L, R, dn, eh, ew, *p, fc, wk, focal, use_override, bw, bs, out, dense, d_w2)) {
    HIPCHK(hipGetLastError());
    return 0;
  }
  { int rcx = pix_exclusive(c); if (rcx) return rcx; }   // gL / gR / gLR are shared by the context's pixel streams
  // E1 refused the FIT only (a fractional or up-scaling INTER_AREA ratio, the VR canvas): it still runs -- 1:1 into a side-by-side scratch of
  // sharpened eyes -- and the fit / mux kernel reads that instead of sharpening two graded planes itself (round 4; same bytes:
  // tests/test_hip_widen.py runs both ways)
  bool taps_ok = (g_fused_fit & 1) != 0;
  for (int l = 0; l < fc.nlev; ++l) if (fc.ksz[l] > 9 || fc.ksz[l] < 3) taps_ok = false;
  if (taps_ok && (p->warp_w & 3) == 0) {
    vd3d_render_params q = *p;
    q.format = VD3D_FMT_HALF_SBS; q.fit_w = p->warp_w; q.fit_h = p->warp_h; q.out_w = 2 * p->warp_w; q.out_h = p->warp_h;
    const size_t need = (size_t)6 * p->warp_w * p->warp_h;
    if (c->gLR_cap < need) { HIPCHK(hipDeviceSynchronize()); HIPCHK(re_alloc(&c->gLR, need)); c->gLR_cap = need; }
    if (vd_launch_finish_fused(c->stream, L, R, dn, eh, ew, q, fc, wk, focal, use_override, bw, bs, c->gLR, dense, d_w2)) {
      vd_launch_sharp_mux(c->stream, c->gLR, c->gLR + (size_t)3 * p->warp_w, *p, fc, out, 2 * p->warp_w);
      HIPCHK(hipGetLastError());
      return 0;
    }
  }
  const float* d_wk = nullptr;
  if (dense) {   // k_dof_grade4's weights: [level][row][32] device table, looked up / built like d_w2 above
    auto same = [&](const vd3d_ctx::wk_tab& t) { return memcmp(t.ksz, fc.ksz, sizeof fc.ksz) == 0 && memcmp(t.kern, fc.kern, sizeof fc.kern) == 0; };
    if (c->wk_cur < 0 || !same(c->wk_tabs[c->wk_cur])) {
      c->wk_cur = -1;
      for (size_t i = 0; i < c->wk_tabs.size(); ++i) if (same(c->wk_tabs[i])) c->wk_cur = (int)i;
      if (c->wk_cur < 0) {
        if (c->wk_tabs.size() >= 64) {
          HIPCHK(hipDeviceSynchronize());
          for (auto& t : c->wk_tabs) (void)hipFree(t.dev);
          c->wk_tabs.clear();
        }
        vd3d_ctx::wk_tab t;
        memcpy(t.ksz, fc.ksz, sizeof fc.ksz); memcpy(t.kern, fc.kern, sizeof fc.kern);
        std::vector<float> host(VD_D4_WTAB_FLOATS, 0.f);
        for (int l = 0; l < fc.nlev; ++l)
          for (int i = 0; i < fc.ksz[l]; ++i)
            for (int j = 0; j < fc.ksz[l]; ++j) host[((size_t)l * 31 + i) * 32 + j] = fc.kern[l][i] * fc.kern[l][j];   // float32 product, as torchvision's outer product holds it
        HIPCHK(hipMalloc((void**)&t.dev, sizeof(float) * VD_D4_WTAB_FLOATS));
        HIPCHK(hipMemcpy(t.dev, host.data(), sizeof(float) * VD_D4_WTAB_FLOATS, hipMemcpyHostToDevice));   // a fresh buffer: nothing queued reads it yet
        c->wk_tabs.push_back(t);
        c->wk_cur = (int)c->wk_tabs.size() - 1;
      }
    }
    d_wk = c->wk_tabs[c->wk_cur].dev;
  }
  if (dense) vd_launch_dof_grade_dense(c->stream, L, R, dn, eh, ew, p->warp_h, p->warp_w, fc, wk, focal, use_override, bw, bs, c->gL, c->gR, d_wk);   // both eyes per launch (round 6)
  else {
    vd_launch_dof_grade(c->stream, L, dn, eh, ew, p->warp_h, p->warp_w, fc, wk, focal, use_override, bw, bs, c->gL, dense, d_wk);
    vd_launch_dof_grade(c->stream, R, dn, eh, ew, p->warp_h, p->warp_w, fc, wk, focal, use_override, bw, bs, c->gR, dense, d_wk);
  }
  // graded planes -> sharpen + fit + mux: the fused kernel's epilogue as a kernel of its own where its fit conditions hold, else the per-pixel one
  if (!((g_fused_fit & 2) && vd_launch_sharp_fit(c->stream, c->gL, c->gR, *p, fc, out))) vd_launch_sharp_mux(c->stream, c->gL, c->gR, *p, fc, out);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_finish_frame(vd3d_ctx* c, const uint8_t* left_bgr, const uint8_t* right_bgr, const float* depth_norm,
                                  int eye_h, int eye_w, const vd3d_render_params* p, double focal_depth, int bar_width,
                                  int bar_side, uint8_t* out_bgr) {
  if (!c || !left_bgr || !right_bgr || !depth_norm || !p || !out_bgr) return set_err(VD3D_E_INVALID, "NULL argument");
  int rc = check_fit(p);
  if (rc) return rc;
  vd_finish_consts fc;
  if ((rc = make_finish_consts(p, &fc))) return rc;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = join_pixels(c))) return rc;
  if ((rc = ensure_work(c, p->warp_h, p->warp_w))) return rc;
  return run_finish(c, left_bgr, right_bgr, depth_norm, eye_h, eye_w, p, fc, (float)focal_depth, 1, bar_width, bar_side, out_bgr);
}

// ---- B2 ---------------------------------------------------------------------------------------
static int render_frame_impl(vd3d_ctx* c, const uint8_t* frame_bgr, const void* depth, int depth_fmt,
                             const vd3d_render_params* p, uint8_t* out_bgr, bool blank) {
  if (!c || !depth || !p || !frame_bgr || !out_bgr) return set_err(VD3D_E_INVALID, "NULL argument");
  if (depth_fmt < 0 || depth_fmt > VD3D_DEPTH_GRAY_U8) return set_err(VD3D_E_INVALID, "bad depth_fmt %d", depth_fmt);
  if (!p->auto_crop_black_bars &&
      (p->crop_x < 0 || p->crop_y < 0 || p->crop_w < 1 || p->crop_h < 1 || p->crop_x + p->crop_w > p->src_w || p->crop_y + p->crop_h > p->src_h))
    return set_err(VD3D_E_INVALID, "crop window outside the frame");
  if (p->auto_crop_black_bars && (!(p->target_ratio > 0.0) || p->src_w < 1 || p->src_h < 1))
    return set_err(VD3D_E_INVALID, "auto_crop_black_bars needs target_ratio > 0");
  if (p->eye_w < 2 || p->eye_h < 2) return set_err(VD3D_E_INVALID, "eye size too small");
  int rc = check_fit(p);
  if (rc) return rc;
  // blank frame: the source-sized frame itself goes through sharpen / fit / mux (:1279-1281, :1406-1419)
  vd3d_render_params pb = *p;
  if (blank) {
    pb.warp_w = p->src_w; pb.warp_h = p->src_h;
    if (p->src_w < 1 || p->src_h < 1) return set_err(VD3D_E_INVALID, "bad source size");
    if ((rc = check_fit(&pb))) return rc;
  }
  // render_sbs_3d forwards literals for the pop/lock controls and never forwards parallax_balance (:1284-1331)
  vd3d_shift_params sp = p->shift;
  sp.parallax_balance = 0.8; sp.depth_pop_gamma = 0.85; sp.depth_pop_mid = 0.50; sp.depth_stretch_lo = 0.05;
  sp.depth_stretch_hi = 0.95; sp.fg_pop_multiplier = 1.20; sp.bg_push_multiplier = 1.10; sp.subject_lock_strength = 1.00;
  sp.aten_threads = p->aten_sum_threads;   // ATen's scalar tails for the same reference process (include/vd3d.h)
  if ((rc = check_shift_params(&sp, p->warp_h, p->warp_w))) return rc;
  vd_finish_consts fc;
  if ((rc = make_finish_consts(p, &fc))) return rc;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = join_pixels(c))) return rc;   // the unsharded pixel pass shares L / R / S with overlapped ones
  if ((rc = ensure_eye(c, p->eye_h, p->eye_w))) return rc;
  if ((rc = ensure_work(c, p->warp_h, p->warp_w))) return rc;
  hipStream_t s = c->stream;
  const long long ne = (long long)p->eye_h * p->eye_w;
  StageTimer tf(c, "frame");
  vd_stage_args a;
  memset(&a, 0, sizeof a);
  a.have_eye = 1; a.W = p->warp_w; a.H = p->warp_h; a.n_eye = ne;
  { const char* e = getenv("VD3D_DBG"); a.dbg = e ? atoi(e) : 0; }
  a.blank = blank ? 1 : 0;
  a.n_crop = (long long)(p->eye_h * 3 / 4 - p->eye_h / 4) * (long long)(p->eye_w * 3 / 4 - p->eye_w / 4);
  a.ipd_factor = p->ipd_factor; a.shift = sp;
  if ((rc = aten_setup(c, p, &a))) return rc;
  float* dn_cur = c->dn[c->dn_cur];
  if (p->auto_crop_black_bars) {   // :1230-1248 decided on device, no host round trip
    if (p->src_h > c->rowflag_cap) { HIPCHK(re_alloc(&c->rowflag, (size_t)p->src_h)); c->rowflag_cap = p->src_h; }
    vd_launch_autocrop(s, frame_bgr, p->src_h, p->src_w, p->target_ratio, c->rowflag, c->work);
    c->crop_scalars_dirty = true;
  } else if (c->crop_scalars_dirty) {
    HIPCHK(hipMemsetAsync(&c->work->fs.crop_top, 0, 2 * sizeof(int32_t), s));
    c->crop_scalars_dirty = false;
  }
  {
    StageTimer t(c, "select_eye");   // fused chain: ingest (+A0), b0 (B0); eye stats ride on the next launch
    HIPCHK(hipMemsetAsync(c->histA, 0, c->hist_bytes, s));
    vd_batch b = batch_of_one(c);
    b.f[0].frame = frame_bgr; b.f[0].depth = depth;
    vd_launch_chain_eye(s, b, depth_fmt, *p, a);
  }
  // a blank frame still runs the whole select chain (its eye-res half carries the filters and the bars; the work-res half only
  // computes unused pop-shaping constants -- blank frames are rare and this keeps one code path), but no shift map and no warp
  rc = run_shift_and_warp(c, c->rgb_eye, dn_cur, p->eye_h, p->eye_w, p->warp_w, p->warp_h, sp, a, blank);
  if (rc) return rc;
  if (blank) {
    StageTimer t(c, "finish");
    const size_t nb = (size_t)p->src_h * p->src_w * 3;
    if (nb > c->blank_cap) { HIPCHK(re_alloc(&c->blank_eye, nb)); c->blank_cap = nb; }
    vd_launch_blank_eye(s, frame_bgr, p->src_h, p->src_w, c->work, c->blank_eye);
    vd_launch_sharp_mux(s, c->blank_eye, c->blank_eye, pb, fc, out_bgr);
    HIPCHK(hipGetLastError());
  } else {
    rc = run_finish(c, c->L, c->R, dn_cur, p->eye_h, p->eye_w, p, fc, 0.f, 0, 0, 0, out_bgr);
    if (rc) return rc;
  }
  c->dn_cur ^= 1;
  return 0;
}

VD3D_EXPORT int vd3d_render_frame(vd3d_ctx* c, const uint8_t* frame_bgr, const void* depth, int depth_fmt,
                                  const vd3d_render_params* p, uint8_t* out_bgr) {
  return render_frame_impl(c, frame_bgr, depth, depth_fmt, p, out_bgr, false);
}

// The frame is in the skip_blank_frames set (core/render_3d.py:1046-1060, 1278-1281): both eyes are the raw source frame; the
// depth filters, ShiftSmoother, dynamic parallax scale and the floating-window bars advance, pixel_shift_cuda (FloatingWindowTracker),
// the ipd scaling, the focal tracker, DOF and the colour grade do not run.  Sharpen / fit / mux work on the source-sized frame.
VD3D_EXPORT int vd3d_render_frame_blank(vd3d_ctx* c, const uint8_t* frame_bgr, const void* depth, int depth_fmt,
                                        const vd3d_render_params* p, uint8_t* out_bgr) {
  return render_frame_impl(c, frame_bgr, depth, depth_fmt, p, out_bgr, true);
}

// ---- frame sharding, three-phase protocol (visiondepth3d_amd/sharded.py) ----------------------------------
VD3D_EXPORT int vd3d_shard_begin(vd3d_ctx* c, const vd3d_render_params* p, int n_slots) {
  if (!c || !p || n_slots < 1 || n_slots > VD_MAX_STEP) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_eye(c, p->eye_h, p->eye_w))) return rc;
  if ((rc = ensure_work(c, p->warp_h, p->warp_w))) return rc;
  const bool same = c->n_slots >= n_slots && c->slot_eh == p->eye_h && c->slot_ew == p->eye_w && c->slot_H == p->warp_h && c->slot_W == p->warp_w;
  if (same) return 0;
  if (c->pix_stream) HIPCHK(hipStreamSynchronize(c->pix_stream));
  for (int k = 0; k < VD_MAX_PIX - 1; ++k) { if (c->pix_x[k]) HIPCHK(hipStreamSynchronize(c->pix_x[k])); c->pix_pending_x[k] = false; }
  c->pix_pending = false; c->excl_set = false; std::fill(c->slot_busy.begin(), c->slot_busy.end(), 0);
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto q : c->slot_rgb) (void)hipFree(q);
  for (auto q : c->slot_dn) (void)hipFree(q);
  for (auto q : c->slot_D) (void)hipFree(q);
  for (auto q : c->slot_tdf) (void)hipFree(q);
  for (auto q : c->slot_tdfp) (void)hipFree(q);
  c->slot_rgb.clear(); c->slot_dn.clear(); c->slot_D.clear(); c->slot_tdf.clear(); c->slot_tdfp.clear();
  for (auto q : c->bdc) (void)hipFree(q);
  c->bdc.clear();
  if (c->bhist) { (void)hipFree(c->bhist); c->bhist = nullptr; }
  c->n_batch = 0;
  const size_t ne = (size_t)p->eye_h * p->eye_w, n = (size_t)p->warp_h * p->warp_w;
  for (int i = 0; i < n_slots; ++i) {
    float *a = nullptr, *b = nullptr, *d = nullptr, *t0 = nullptr, *t1 = nullptr;
    HIPCHK(hipMalloc((void**)&a, 3 * ne * sizeof(float))); HIPCHK(hipMalloc((void**)&b, ne * sizeof(float)));
    HIPCHK(hipMalloc((void**)&d, n * sizeof(float)));
    HIPCHK(hipMalloc((void**)&t0, ne * sizeof(float))); HIPCHK(hipMalloc((void**)&t1, ne * sizeof(float)));
    c->slot_rgb.push_back(a); c->slot_dn.push_back(b); c->slot_D.push_back(d); c->slot_tdf.push_back(t0); c->slot_tdfp.push_back(t1);
  }
  if (!c->etab) HIPCHK(hipMalloc((void**)&c->etab, (size_t)(VD_MAX_STEP + 1) * VD_ETAB * sizeof(float)));
  if (!c->crop_tab) HIPCHK(hipMalloc((void**)&c->crop_tab, (size_t)VD_MAX_STEP * 4 * sizeof(int)));
  HIPCHK(re_alloc(&c->slot_work, (size_t)n_slots));
  c->slot_prev.assign((size_t)n_slots, nullptr);
  for (int i = 0; i < n_slots; ++i) c->slot_prev[i] = c->slot_tdfp[i];
  c->n_batch = n_slots < VD_MAX_BATCH ? n_slots : VD_MAX_BATCH;
  HIPCHK(hipMalloc((void**)&c->bhist, (size_t)c->n_batch * c->hist_bytes));
  for (int i = 0; i < c->n_batch; ++i) { float* q = nullptr; HIPCHK(hipMalloc((void**)&q, n * sizeof(float))); c->bdc.push_back(q); }
  c->n_slots = n_slots; c->slot_eh = p->eye_h; c->slot_ew = p->eye_w; c->slot_H = p->warp_h; c->slot_W = p->warp_w;
  return 0;
}
// phase 3: shift plane, fused warp and finishing kernels of one owned frame from its slot -> muxed frame
static int shard_pixels_impl(vd3d_ctx* c, int slot, const vd3d_render_params* p, uint8_t* out_bgr, const uint8_t* blank_frame_bgr) {
  if (!c || !p || !out_bgr || slot < 0 || slot >= c->n_slots) return set_err(VD3D_E_INVALID, "bad argument");
  int rc = check_fit(p);
  if (rc) return rc;
  vd3d_render_params pb = *p;
  if (blank_frame_bgr) {   // the source-sized frame itself goes through sharpen / fit / mux (:1279-1281, :1406-1419)
    pb.warp_w = p->src_w; pb.warp_h = p->src_h;
    if (p->src_w < 1 || p->src_h < 1) return set_err(VD3D_E_INVALID, "bad source size");
    if ((rc = check_fit(&pb))) return rc;
  }
  vd3d_shift_params sp = p->shift;
  sp.parallax_balance = 0.8; sp.depth_pop_gamma = 0.85; sp.depth_pop_mid = 0.50; sp.depth_stretch_lo = 0.05;
  sp.depth_stretch_hi = 0.95; sp.fg_pop_multiplier = 1.20; sp.bg_push_multiplier = 1.10; sp.subject_lock_strength = 1.00;
  sp.aten_threads = p->aten_sum_threads;   // ATen's scalar tails for the same reference process (include/vd3d.h)
  vd_finish_consts fc;
  if ((rc = make_finish_consts(p, &fc))) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (p->warp_h != c->slot_H || p->warp_w != c->slot_W || p->eye_h != c->slot_eh || p->eye_w != c->slot_ew)
    return set_err(VD3D_E_INVALID, "vd3d_shard_pixels: %dx%d (eye %dx%d) is not the size of vd3d_shard_begin (%dx%d, eye %dx%d)", p->warp_w, p->warp_h,
                   p->eye_w, p->eye_h, c->slot_W, c->slot_H, c->slot_ew, c->slot_eh);
  if (c->H != p->warp_h || c->W != p->warp_w) {
    // another entry point (vd3d_pixel_shift / vd3d_render_frame at another size) re-sized the context's shared warp-res planes since
    // vd3d_shard_begin: bring them back before a pixel pass writes H x W planes into them (hipFree synchronises the device)
    if ((rc = join_pixels(c))) return rc;
    if ((rc = ensure_work(c, p->warp_h, p->warp_w))) return rc;
  }
  // overlapped mode: this pass runs on pix_stream behind everything enqueued on the main stream so far (the slot's measurements and
  // the replay that patched its constants); the main stream is free to start the next step's measurement chain meanwhile
  struct StreamSwap {
    vd3d_ctx* c; hipStream_t saved;
    explicit StreamSwap(vd3d_ctx* ctx) : c(ctx), saved(ctx->stream) {}
    ~StreamSwap() { c->stream = saved; c->cur_pix = -1; c->cur_excl = false; }
  } swap(c);
  const int H = p->warp_h, W = p->warp_w;
  int k = 0;
  float* S = c->S; uint8_t* L = c->L; uint8_t* R = c->R; float* E2 = c->E2;
  if (c->pix_overlap) {
    while ((int)c->slot_done.size() <= slot) {
      hipEvent_t e;
      HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      c->slot_done.push_back(e); c->slot_busy.push_back(0);
    }
    if (c->n_pix > 1 && !blank_frame_bgr) {
      k = (int)(c->pix_rr++ % (unsigned)c->n_pix);
      if (c->x_H != H || c->x_W != W) {   // the extra streams' planes follow the warp size (rare: drain them first)
        for (int j = 0; j < VD_MAX_PIX - 1; ++j) {
          if (c->pix_x[j]) HIPCHK(hipStreamSynchronize(c->pix_x[j]));
          HIPCHK(re_alloc(&c->S_x[j], (size_t)0)); HIPCHK(re_alloc(&c->L_x[j], (size_t)0)); HIPCHK(re_alloc(&c->R_x[j], (size_t)0));
          HIPCHK(re_alloc(&c->E2_x[j], (size_t)0));
        }
        c->x_H = H; c->x_W = W;
      }
      if (k > 0) {
        const size_t n = (size_t)H * W;
        if (!c->S_x[k - 1]) {
          HIPCHK(re_alloc(&c->S_x[k - 1], n)); HIPCHK(re_alloc(&c->L_x[k - 1], 3 * n)); HIPCHK(re_alloc(&c->R_x[k - 1], 3 * n));
          HIPCHK(re_alloc(&c->E2_x[k - 1], 2 * n));
        }
        S = c->S_x[k - 1]; L = c->L_x[k - 1]; R = c->R_x[k - 1]; E2 = c->E2_x[k - 1];
      }
    }
    hipStream_t sk = k == 0 ? c->pix_stream : c->pix_x[k - 1];
    HIPCHK(hipEventRecord(c->ev_chain, c->stream));
    HIPCHK(hipStreamWaitEvent(sk, c->ev_chain, 0));
    if (c->excl_set) HIPCHK(hipStreamWaitEvent(sk, c->ev_excl, 0));   // a pass that used the shared fallback planes is still the latest such user
    c->stream = sk;
    c->cur_pix = k; c->cur_excl = false;
    if (blank_frame_bgr) { int rcx = pix_exclusive(c); if (rcx) return rcx; }   // blank_eye is a shared plane
  }
  hipStream_t s = c->stream;
  const vd_dev_work* wk = &c->slot_work[slot];
  if (blank_frame_bgr) {
    StageTimer t(c, "finish");
    const size_t nb = (size_t)p->src_h * p->src_w * 3;
    if (nb > c->blank_cap) { HIPCHK(re_alloc(&c->blank_eye, nb)); c->blank_cap = nb; }
    vd_launch_blank_eye(s, blank_frame_bgr, p->src_h, p->src_w, wk, c->blank_eye);
    vd_launch_sharp_mux(s, c->blank_eye, c->blank_eye, pb, fc, out_bgr);
    HIPCHK(hipGetLastError());
  } else {
  { StageTimer t(c, "warp");
    // fused path with feathering: k_e2w writes the gradient mask of both eyes, W1 starts at its window sums
    const vd3d_shift_params spw = warp_stage_params(sp);   // feather_strength <= 0 (the GUI's default): W1 without mask, window sums and blend -- exact
    const float* rgb = c->slot_rgb[slot];
    int rih = p->eye_h, riw = p->eye_w;
    if (!(rih == H && riw == W) && vd_interp_premult(3, H, W, sp.aten_threads)) {   // N-thread ATen mode: the eye -> warp resize of :595 by ATen's other kernel
      if ((rc = pix_exclusive(c))) return rc;
      if ((rc = premult_resize(c, 3, &rgb, &rih, &riw, H, W, sp.aten_threads, &c->pm_rgb, &c->pm_rgb_cap))) return rc;
    }
    const bool pre = spw.enable_feathering && vd_warp_fused_ok(rih, riw, H, W, spw);
    // without feathering W1 computes the shift values of its own tile (round 6): no k_shift launch, no S plane (8 N bytes of traffic less)
    const bool fold = vd_warp_fold_ok(rih, riw, H, W, spw, sp);
    const vd_shift_fold ff = {wk, sp, nullptr};
    if (!fold) { StageTimer t1(c, "shift"); vd_launch_shift(s, c->slot_D[slot], H, W, wk, sp, S); }
    bool fused;
    { StageTimer t2(c, "w1");
      if (pre) { StageTimer t3(c, "e2w"); vd_launch_e2w(s, c->slot_D[slot], S, H, W, (float)spw.feather_strength, E2); }
      fused = vd_launch_warp_fused(s, rgb, rih, riw, c->slot_D[slot], S, H, W, spw, L, R, pre ? E2 : nullptr, fold ? &ff : nullptr); }
    if (!fused && fold) { StageTimer t1(c, "shift"); vd_launch_shift(s, c->slot_D[slot], H, W, wk, sp, S); }
    if (!fused) {
      if ((rc = pix_exclusive(c))) return rc;
      if (spw.enable_feathering) {
        vd_launch_e2(s, c->slot_D[slot], S, H, W, (float)spw.feather_strength, c->e2L, c->e2R);
        vd_launch_pool(s, c->e2L, c->e2R, H, W, spw.blur_ksize, c->bL, c->bR);
      }
      vd_launch_warp(s, rgb, rih, riw, S, c->bL, c->bR, H, W, spw.enable_feathering ? 1 : 0, L, R);
    }
  }
  HIPCHK(hipGetLastError());
  rc = run_finish(c, L, R, c->slot_dn[slot], p->eye_h, p->eye_w, p, fc, 0.f, 0, 0, 0, out_bgr, wk);
  if (rc) return rc;
  }
  if (c->pix_overlap) {
    HIPCHK(hipEventRecord(c->slot_done[slot], c->stream));
    if (k == 0) { HIPCHK(hipEventRecord(c->ev_pix_last, c->stream)); c->pix_pending = true; }
    else { HIPCHK(hipEventRecord(c->ev_pix_last_x[k - 1], c->stream)); c->pix_pending_x[k - 1] = true; }
    if (c->cur_excl) { HIPCHK(hipEventRecord(c->ev_excl, c->stream)); c->excl_set = true; }
    c->slot_busy[slot] = 1;
  }
  return 0;
}

VD3D_EXPORT int vd3d_shard_pixels(vd3d_ctx* c, int slot, const vd3d_render_params* p, uint8_t* out_bgr) {
  return shard_pixels_impl(c, slot, p, out_bgr, nullptr);
}
// the pixel pass of an own frame that is in the skip_blank_frames set (core/render_3d.py:1278-1281): both eyes are the source frame
VD3D_EXPORT int vd3d_shard_pixels_blank(vd3d_ctx* c, int slot, const uint8_t* frame_bgr, const vd3d_render_params* p, uint8_t* out_bgr) {
  if (!frame_bgr) return set_err(VD3D_E_INVALID, "NULL frame");
  return shard_pixels_impl(c, slot, p, out_bgr, frame_bgr);
}

// Overlapped pixel passes: with enable != 0, vd3d_shard_pixels is enqueued on a second stream of the context, ordered after all work
// enqueued so far, and returns; the measurement chain of the NEXT step (vd3d_shard2_p1 ... r2, latency-bound) then runs concurrently with
// the pixel kernels of this one.  Slots are guarded: a call that overwrites a slot first waits for the pixel pass that still reads it, so
// a caller that alternates between two slot sets gets the overlap and a caller that does not gets the sequential order.  Outputs are
// complete after vd3d_sync, or, for consumers ordered on the context's stream, after vd3d_join_pixels.
VD3D_EXPORT int vd3d_set_pixel_overlap(vd3d_ctx* c, int enable) {
  if (!c) return set_err(VD3D_E_INVALID, "NULL context");
  if (enable < 0 || enable > VD_MAX_PIX) return set_err(VD3D_E_INVALID, "vd3d_set_pixel_overlap: 0 (off) or 1 .. %d pixel streams", VD_MAX_PIX);
  HIPCHK(hipSetDevice(c->device));
  int rc = join_pixels(c);
  if (rc) return rc;
  if (enable && !c->pix_stream) {
    HIPCHK(hipStreamCreateWithFlags(&c->pix_stream, hipStreamNonBlocking));   // stream priorities: measured, no effect either way
    HIPCHK(hipEventCreateWithFlags(&c->ev_chain, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_pix_last, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_excl, hipEventDisableTiming));
  }
  for (int k = 1; k < enable; ++k)
    if (!c->pix_x[k - 1]) {
      HIPCHK(hipStreamCreateWithFlags(&c->pix_x[k - 1], hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&c->ev_pix_last_x[k - 1], hipEventDisableTiming));
    }
  c->pix_overlap = enable != 0;
  c->n_pix = enable > 1 ? enable : 1;
  return 0;
}
VD3D_EXPORT int vd3d_join_pixels(vd3d_ctx* c) {
  if (!c) return set_err(VD3D_E_INVALID, "NULL context");
  HIPCHK(hipSetDevice(c->device));
  return join_pixels(c);
}
// host-side wait for the overlapped pixel pass of one slot (its output frame is then complete); no-op if none is outstanding
VD3D_EXPORT int vd3d_wait_pixels(vd3d_ctx* c, int slot) {
  if (!c || slot < 0) return set_err(VD3D_E_INVALID, "bad argument");
  // not gated on slot_busy: a later chain call may already have ordered the first stream behind this pass (clearing the flag)
  // while the host has not waited yet; synchronising a completed or never-recorded event returns at once
  if (slot < (int)c->slot_done.size()) HIPCHK(hipEventSynchronize(c->slot_done[slot]));
  return 0;
}


// ---- frame sharding, measure / replay protocol (visiondepth3d_amd/sharded.py: MeasureReplaySharder) ----------
// Replicated work per foreign frame = ONE small kernel (the TemporalDepthFilter plane EMA); everything else is measured by the
// owner, exchanged as a few numbers per frame and replayed as scalar recurrences on every rank.
static int shard2_args(vd3d_ctx* c, const vd3d_render_params* p, vd_stage_args* a, vd3d_shift_params* sp) {
  *sp = p->shift;
  sp->parallax_balance = 0.8; sp->depth_pop_gamma = 0.85; sp->depth_pop_mid = 0.50; sp->depth_stretch_lo = 0.05;
  sp->depth_stretch_hi = 0.95; sp->fg_pop_multiplier = 1.20; sp->bg_push_multiplier = 1.10; sp->subject_lock_strength = 1.00;
  sp->aten_threads = p->aten_sum_threads;
  memset(a, 0, sizeof *a);
  a->have_eye = 1; a->W = p->warp_w; a->H = p->warp_h; a->n_eye = (long long)p->eye_h * p->eye_w;
  a->n_crop = (long long)(p->eye_h * 3 / 4 - p->eye_h / 4) * (long long)(p->eye_w * 3 / 4 - p->eye_w / 4);
  a->ipd_factor = p->ipd_factor; a->shift = *sp; a->etab = c->etab;
  { static int dbg = -1; if (dbg < 0) { const char* e = getenv("VD3D_DBG"); dbg = e ? atoi(e) : 0; } a->dbg = dbg; }   // timing probes only (vd3d_kernels.h)
  return aten_setup(c, p, a);
}
// P1, for every OWN frame of the step in frame order (a rank owns a contiguous chunk of the step): ingest (RGB kept in the slot),
// TemporalDepthFilter plane EMA, exact q.02 / q.98 of the filtered plane written to q_out_dev[0..1]; the filtered planes of this
// frame and of the frame before it are kept in the slot.  The plane EMA carries over from the previous frame of the clip, wherever
// it was rendered: vd3d_tdf_plane_import installs the plane the previous chunk's owner exported.
// Batched form: n consecutive own frames (slots slot0 .. slot0 + n - 1, step indices step_idx0 ..) in TWO launches -- K1 walks the
// frames inside every workgroup (the EMA is a per-pixel recurrence), K2 runs the frames side by side; per-launch costs are paid once.
static int shard2_p1_impl(vd3d_ctx* c, const uint8_t* const* frames_bgr, const void* const* depths, int depth_fmt, const vd3d_render_params* p,
                          int step_idx0, int slot0, int n, float* q_out_dev) {
  if (!c || !frames_bgr || !depths || !p || !q_out_dev || n < 1 || step_idx0 < 0 || step_idx0 + n > VD_MAX_STEP) return set_err(VD3D_E_INVALID, "bad argument");
  if (slot0 < 0 || slot0 + n > c->n_slots) return set_err(VD3D_E_INVALID, "slots %d..%d out of range (vd3d_shard_begin)", slot0, slot0 + n - 1);
  if (n > c->n_batch) return set_err(VD3D_E_INVALID, "batch of %d frames > %d", n, c->n_batch);
  for (int j = 0; j < n; ++j) if (!frames_bgr[j] || !depths[j]) return set_err(VD3D_E_INVALID, "an own frame needs the frame and its depth plane");
  if (depth_fmt < 0 || depth_fmt > VD3D_DEPTH_GRAY_U8) return set_err(VD3D_E_INVALID, "bad depth_fmt %d", depth_fmt);
  if (p->auto_crop_black_bars && !c->crop_tab_set)
    return set_err(VD3D_E_INVALID, "auto_crop_black_bars in a sharded step: call vd3d_shard2_p0 on the own frames and vd3d_shard2_set_crops first");
  HIPCHK(hipSetDevice(c->device));
  for (int j = 0; j < n; ++j) { int rcw = wait_slot(c, slot0 + j); if (rcw) return rcw; }
  hipStream_t s = c->stream;
  vd_stage_args a; vd3d_shift_params sp;
  { int rca = shard2_args(c, p, &a, &sp); if (rca) return rca; }
  a.crop_tab = p->auto_crop_black_bars ? c->crop_tab : nullptr;
  const size_t ne = (size_t)p->eye_h * p->eye_w;
  StageTimer t(c, "p1_own");
  a.shard = 3;
  // the plane before the first frame of the batch is the context's filter state; inside the batch every frame reads its predecessor's slot
  HIPCHK(hipMemcpyAsync(c->slot_tdfp[slot0], c->tdf, ne * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemsetAsync(&c->slot_work[slot0], 0, (size_t)n * sizeof(vd_dev_work), s));   // tickets, fixed-point sums, select jobs of the frames
  HIPCHK(hipMemsetAsync(c->bhist, 0, (size_t)n * c->hist_bytes, s));
  vd_batch b;
  memset(&b, 0, sizeof b);
  b.n = n; b.w_main = c->work;
  const size_t nA = (size_t)VD_NJOBS * VD_NB_A;
  for (int j = 0; j < n; ++j) {
    vd_batch_frame& F = b.f[j];
    const int slot = slot0 + j;
    F.w = &c->slot_work[slot];
    F.histA = c->bhist + (size_t)j * (c->hist_bytes / sizeof(uint32_t)); F.histB = F.histA + nA;
    F.frame = frames_bgr[j]; F.depth = depths[j];
    F.rgb_eye = c->slot_rgb[slot]; F.tdf = c->slot_tdf[slot];
    F.tdf_prev = j == 0 ? c->slot_tdfp[slot0] : c->slot_tdf[slot - 1];
    c->slot_prev[slot] = F.tdf_prev;
    F.q_out = q_out_dev + 2 * j; F.shard_idx = step_idx0 + j;
  }
  vd_launch_chain_eye(s, b, depth_fmt, *p, a);
  HIPCHK(hipMemcpyAsync(c->tdf, c->slot_tdf[slot0 + n - 1], ne * sizeof(float), hipMemcpyDeviceToDevice, s));   // the filter state after the batch
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_shard2_p1(vd3d_ctx* c, const uint8_t* frame_bgr, const void* depth, int depth_fmt, const vd3d_render_params* p,
                               int step_idx, int slot, float* q_out_dev) {
  return shard2_p1_impl(c, &frame_bgr, &depth, depth_fmt, p, step_idx, slot, 1, q_out_dev);
}
VD3D_EXPORT int vd3d_shard2_p1_batch(vd3d_ctx* c, const uint8_t* const* frames_bgr, const void* const* depths, int depth_fmt,
                                     const vd3d_render_params* p, int step_idx0, int slot0, int n, float* q_out_dev) {
  return shard2_p1_impl(c, frames_bgr, depths, depth_fmt, p, step_idx0, slot0, n, q_out_dev);
}
// The chunk hand-off of the plane state (one eye-size float32 plane per chunk boundary): export copies
// TemporalDepthFilter.prev_depth to a caller buffer (which the caller sends to the owner of the next chunk), import installs a
// received plane and marks it valid (valid = 0: "no previous frame", the state of a fresh clip).
VD3D_EXPORT int vd3d_tdf_plane_export(vd3d_ctx* c, float* dst_dev, int eye_h, int eye_w) {
  if (!c || !dst_dev || !c->tdf || eye_h != c->eye_h || eye_w != c->eye_w) return set_err(VD3D_E_INVALID, "bad argument (vd3d_shard_begin first)");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(dst_dev, c->tdf, (size_t)eye_h * eye_w * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}
VD3D_EXPORT int vd3d_tdf_plane_import(vd3d_ctx* c, const float* src_dev, int eye_h, int eye_w, int valid) {
  if (!c || !src_dev || !c->tdf || eye_h != c->eye_h || eye_w != c->eye_w) return set_err(VD3D_E_INVALID, "bad argument (vd3d_shard_begin first)");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->tdf, src_dev, (size_t)eye_h * eye_w * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  const int32_t v = valid ? 1 : 0;
  HIPCHK(hipMemcpyAsync(&c->work->st.tdf_valid, &v, sizeof v, hipMemcpyHostToDevice, c->stream));   // pageable 4-byte source: staged by the runtime
  return 0;
}
// P0 (only with auto_crop_black_bars), own frames: detect_black_bars + the per-frame aspect crop -> crop_out_dev[0..3] = {x, y, w, h}.
// The rectangles of ALL frames of the step are then all-gathered by the caller and installed with vd3d_shard2_set_crops.
VD3D_EXPORT int vd3d_shard2_p0(vd3d_ctx* c, const uint8_t* frame_bgr, const vd3d_render_params* p, int* crop_out_dev) {
  if (!c || !frame_bgr || !p || !crop_out_dev) return set_err(VD3D_E_INVALID, "NULL argument");
  if (!(p->target_ratio > 0.0) || p->src_w < 1 || p->src_h < 1) return set_err(VD3D_E_INVALID, "auto_crop_black_bars needs target_ratio > 0");
  HIPCHK(hipSetDevice(c->device));
  if (p->src_h > c->rowflag_cap) { HIPCHK(re_alloc(&c->rowflag, (size_t)p->src_h)); c->rowflag_cap = p->src_h; }
  vd_launch_autocrop(c->stream, frame_bgr, p->src_h, p->src_w, p->target_ratio, c->rowflag, c->work, crop_out_dev);
  c->crop_scalars_dirty = true;
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_shard2_set_crops(vd3d_ctx* c, const int* crops_all_dev, int n) {
  if (!c || !crops_all_dev || n < 1 || n > VD_MAX_STEP || !c->crop_tab) return set_err(VD3D_E_INVALID, "bad argument (vd3d_shard_begin first)");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->crop_tab, crops_all_dev, (size_t)n * 4 * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  c->crop_tab_set = true;
  return 0;
}
// R1: replay DepthPercentileEMA over the n frames of the step from the exchanged quantiles q_all_dev[n][2] (frame order)
VD3D_EXPORT int vd3d_shard2_r1(vd3d_ctx* c, const float* q_all_dev, int n) {
  if (!c || !q_all_dev || n < 1 || n > VD_MAX_STEP || !c->etab) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  vd_launch_shard2_r1(c->stream, c->work, q_all_dev, n, c->etab);
  HIPCHK(hipGetLastError());
  return 0;
}
// P3, own frames only: normalise, eye-res statistics, warp-res select chain, shaped depth plane, s1 -> measurements
// m_out_dev[0..3] = {sum1, sum2, sum_mad, (s_norm | s1 << 32)}; planes and shape constants stay in the slot.
// Batched form: the frames are independent once R1 has replayed the normalisation table, so n frames go through K3a ... K6 side by side
// (five launches per group of `VD3D_CHAIN_GROUP` frames; a group's curved-depth planes stay cache-resident between its launches).
static int g_chain_group = -1;   // frames per group of the batched P3 (VD3D_CHAIN_GROUP / vd3d_debug_tune)
static int shard2_p3_impl(vd3d_ctx* c, int slot0, int step_idx0, int n, const vd3d_render_params* p, long long* m_out_dev) {
  if (!c || !p || !m_out_dev || n < 1 || slot0 < 0 || slot0 + n > c->n_slots || step_idx0 < 0 || step_idx0 + n > VD_MAX_STEP) return set_err(VD3D_E_INVALID, "bad argument");
  if (n > c->n_batch) return set_err(VD3D_E_INVALID, "batch of %d frames > %d", n, c->n_batch);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  vd_stage_args a; vd3d_shift_params sp;
  int rc;
  if ((rc = shard2_args(c, p, &a, &sp))) return rc;
  if ((rc = check_shift_params(&sp, p->warp_h, p->warp_w))) return rc;
  a.shard = 3;
  for (int j = 0; j < n; ++j) if ((rc = wait_slot(c, slot0 + j))) return rc;
  int& group = g_chain_group;
  if (group < 0) { const char* e = getenv("VD3D_CHAIN_GROUP"); group = e ? atoi(e) : VD_MAX_BATCH; }
  if (group < 1) group = 1;
  if (group > VD_MAX_BATCH) group = VD_MAX_BATCH;
  StageTimer t(c, "p3_own");
  const size_t nA = (size_t)VD_NJOBS * VD_NB_A;
  for (int j0 = 0; j0 < n; j0 += group) {
    const int g = n - j0 < group ? n - j0 : group;
    HIPCHK(hipMemsetAsync(c->bhist, 0, (size_t)g * c->hist_bytes, s));   // the select jobs of these frames start from empty histograms
    vd_batch b;
    memset(&b, 0, sizeof b);
    b.n = g; b.w_main = c->work;
    for (int j = 0; j < g; ++j) {
      vd_batch_frame& F = b.f[j];
      const int slot = slot0 + j0 + j;
      F.w = &c->slot_work[slot];
      F.histA = c->bhist + (size_t)j * (c->hist_bytes / sizeof(uint32_t)); F.histB = F.histA + nA;
      F.tdf = c->slot_tdf[slot]; F.dn = c->slot_dn[slot]; F.dn_prev = c->slot_prev[slot];
      F.dc = c->bdc[j]; F.D = c->slot_D[slot];
      F.m_out = m_out_dev + 4 * (j0 + j); F.shard_idx = step_idx0 + j0 + j;
    }
    vd_launch_chain_work(s, b, 1, p->eye_h, p->eye_w, p->warp_h, p->warp_w, (float)sp.depth_pop_mid, (float)sp.depth_pop_gamma, a);
  }
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_shard2_p3(vd3d_ctx* c, int slot, int step_idx, const vd3d_render_params* p, long long* m_out_dev) {
  return shard2_p3_impl(c, slot, step_idx, 1, p, m_out_dev);
}
VD3D_EXPORT int vd3d_shard2_p3_batch(vd3d_ctx* c, int slot0, int step_idx0, int n, const vd3d_render_params* p, long long* m_out_dev) {
  return shard2_p3_impl(c, slot0, step_idx0, n, p, m_out_dev);
}
// R2: replay every remaining tracker over the n frames of the step from the exchanged measurements m_all_dev[n][4] (frame order);
// own_slot_host[t] = slot of frame t on this rank or -1.  Afterwards vd3d_shard_pixels(slot) renders the own frames.
VD3D_EXPORT int vd3d_shard2_r2(vd3d_ctx* c, const long long* m_all_dev, const int* own_slot_host, const uint8_t* blank_host_or_null, int n,
                               const vd3d_render_params* p) {
  if (!c || !m_all_dev || !own_slot_host || !p || n < 1 || n > VD_MAX_STEP) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  vd_stage_args a; vd3d_shift_params sp;
  { int rca = shard2_args(c, p, &a, &sp); if (rca) return rca; }
  for (int t = 0; t < n; ++t) { int rc = wait_slot(c, own_slot_host[t]); if (rc) return rc; }
  StageTimer t(c, "replay");
  vd_launch_shard2_r2(c->stream, c->work, m_all_dev, c->etab, own_slot_host, blank_host_or_null, n, c->slot_work, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- diagnostics / tests --------------------------------------------------------------------------
VD3D_EXPORT int vd3d_debug_planes(vd3d_ctx* c, float** D, float** S, uint8_t** L, uint8_t** R, float** rgb_eye, float** dn_cur) {
  if (D) *D = c->D;
  if (S) *S = c->S;
  if (L) *L = c->L;
  if (R) *R = c->R;
  if (rgb_eye) *rgb_eye = c->rgb_eye;
  if (dn_cur) *dn_cur = c->dn[c->dn_cur ^ 1];  // the plane the last render_frame wrote
  return 0;
}

VD3D_EXPORT int vd3d_quantiles(vd3d_ctx* c, const float* plane, int64_t n, const float* q_host, int nq, float* out_host) {
  if (!c || !plane || !q_host || !out_host || n < 1 || nq < 1) return set_err(VD3D_E_INVALID, "bad argument");
  if (n >= (1ll << 31)) return set_err(VD3D_E_INVALID, "n too large");
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < nq; i += 2) {
    vd_stage_args a;
    memset(&a, 0, sizeof a);
    // reuse the work-res quantile job through the stretch_lo/hi slots
    a.shift.depth_stretch_lo = q_host[i];
    a.shift.depth_stretch_hi = q_host[i + 1 < nq ? i + 1 : i];
    HIPCHK(hipMemsetAsync(c->histA, 0, c->hist_bytes, c->stream));
    vd_launch_hist_eye_d(c->stream, false, plane, n, c->work, c->histA, c->histB);
    a.stage = VD_ST_AQ; vd_launch_scalar_stage(c->stream, c->work, c->histA, c->histB, a);
    vd_launch_hist_eye_d(c->stream, true, plane, n, c->work, c->histA, c->histB);
    a.stage = VD_ST_BQ; vd_launch_scalar_stage(c->stream, c->work, c->histA, c->histB, a);
    float res[2];
    HIPCHK(hipMemcpyAsync(res, &c->work->fs.q_lo, 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out_host[i] = res[0];
    if (i + 1 < nq) out_host[i + 1] = res[1];
  }
  return 0;
}

VD3D_EXPORT int vd3d_subject_depth(vd3d_ctx* c, const float* plane, int H, int W, float* out_host) {
  if (!c || !plane || !out_host || H < 1 || W < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  vd_stage_args a;
  memset(&a, 0, sizeof a);
  HIPCHK(hipMemsetAsync(c->histA, 0, c->hist_bytes, c->stream));
  vd_launch_hist_work_s1(c->stream, false, plane, H, W, c->work, c->histA, c->histB);
  a.stage = VD_ST_A2; vd_launch_scalar_stage(c->stream, c->work, c->histA, c->histB, a);
  vd_launch_hist_work_s1(c->stream, true, plane, H, W, c->work, c->histA, c->histB);
  a.stage = VD_ST_BS; vd_launch_scalar_stage(c->stream, c->work, c->histA, c->histB, a);
  HIPCHK(hipMemcpyAsync(out_host, &c->work->fs.s1, sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// a23: heal_missing_pixels, core/render_3d.py:431-459 (optional stage; the reference's loop never calls it)
VD3D_EXPORT int vd3d_heal_missing_pixels(vd3d_ctx* c, const float* warped_chw, const float* original_chw, const float* edge_mask_or_null,
                                         int H, int W, double heal_strength, float* out_chw) {
  if (!c || !warped_chw || !original_chw || !out_chw || H < 1 || W < 1) return set_err(VD3D_E_INVALID, "bad argument");
  if (out_chw == warped_chw || out_chw == original_chw) return set_err(VD3D_E_INVALID, "out may not alias an input (3x3 neighbourhood reads)");
  if ((long long)H * W * 3 >= (1ll << 31)) return set_err(VD3D_E_INVALID, "frame too large");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "heal");
  vd_launch_heal(c->stream, warped_chw, original_chw, edge_mask_or_null, H, W, (float)heal_strength, out_chw);
  HIPCHK(hipGetLastError());
  return 0;
}

// cv2.resize(u8, (dw, dh), interpolation=cv2.INTER_CUBIC): a24 with an explicit inference size (core/render_depth.py:1917) and the
// up-scale stage's size changes (core/merged_pipeline.py:260-264)
VD3D_EXPORT int vd3d_resize_cubic_u8(vd3d_ctx* c, const uint8_t* src, int sh, int sw, int cn, uint8_t* dst, int dh, int dw) {
  if (!c || !src || !dst || sh < 1 || sw < 1 || dh < 1 || dw < 1 || src == dst) return set_err(VD3D_E_INVALID, "bad argument");
  if ((long long)sh * sw * cn >= (1ll << 31) || (long long)dh * dw * cn >= (1ll << 31)) return set_err(VD3D_E_INVALID, "image too large");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "resize_cubic");
  if (!vd_launch_resize_cubic_u8(c->stream, src, sh, sw, cn, dst, dh, dw)) return set_err(VD3D_E_UNSUPPORTED, "resize_cubic_u8: %d channels (1 or 3)", cn);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_resize_area_u8(vd3d_ctx* c, const uint8_t* src_bgr, int sh, int sw, uint8_t* dst_bgr, int dh, int dw) {
  if (!c || !src_bgr || !dst_bgr || sh < 1 || sw < 1 || dh < 1 || dw < 1 || src_bgr == dst_bgr) return set_err(VD3D_E_INVALID, "bad argument");
  if ((long long)sh * sw * 3 >= (1ll << 31) || (long long)dh * dw * 3 >= (1ll << 31)) return set_err(VD3D_E_INVALID, "image too large");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "resize_area");
  if (!vd_launch_resize_area_u8(c->stream, src_bgr, sh, sw, dst_bgr, dh, dw))
    return set_err(VD3D_E_UNSUPPORTED, "resize_area_u8: %dx%d -> %dx%d exceeds the tap budget (ratio <= 10)", sw, sh, dw, dh);
  HIPCHK(hipGetLastError());
  return 0;
}

// cv2.resize(src, (dw, dh)) -- INTER_LINEAR, OpenCV's default -- on uint8 BGR: format_3d_output's VR branch (core/render_3d.py:846-849)
VD3D_EXPORT int vd3d_resize_linear_u8(vd3d_ctx* c, const uint8_t* src_bgr, int sh, int sw, uint8_t* dst_bgr, int dh, int dw) {
  if (!c || !src_bgr || !dst_bgr || sh < 1 || sw < 1 || dh < 1 || dw < 1 || src_bgr == dst_bgr) return set_err(VD3D_E_INVALID, "bad argument");
  if ((long long)sh * sw * 3 >= (1ll << 31) || (long long)dh * dw * 3 >= (1ll << 31)) return set_err(VD3D_E_INVALID, "image too large");
  HIPCHK(hipSetDevice(c->device));
  vd_launch_resize_linear_u8(c->stream, src_bgr, sh, sw, dst_bgr, dh, dw);
  HIPCHK(hipGetLastError());
  return 0;
}

// format_3d_output(left, right, fmt), core/render_3d.py:837-860, on two uint8 BGR eyes of h x w: Half-/Full-SBS = side by side, VR = both eyes
// resized to 1440 x 1600 (INTER_LINEAR) side by side, Red-Cyan Anaglyph = generate_anaglyph_3d, Passive Interlaced = even rows left / odd rows
// right.  out: [h][2w][3] (SBS), [1600][2880][3] (VR), [h][w][3] (anaglyph, interlaced).  The mux runs through k_sharp_mux with the identity
// sharpen kernel (kc = 1, kn = 0: exact) and a 1:1 fit.
VD3D_EXPORT int vd3d_format_3d_output(vd3d_ctx* c, const uint8_t* left_bgr, const uint8_t* right_bgr, int h, int w, int format, uint8_t* out_bgr) {
  if (!c || !left_bgr || !right_bgr || !out_bgr || h < 1 || w < 1) return set_err(VD3D_E_INVALID, "bad argument");
  if (format < 0 || format > VD3D_FMT_INTERLACED) return set_err(VD3D_E_INVALID, "unknown format %d", format);
  HIPCHK(hipSetDevice(c->device));
  int rc = join_pixels(c);
  if (rc) return rc;
  const uint8_t *L = left_bgr, *R = right_bgr;
  int eh = h, ew = w;
  if (format == VD3D_FMT_VR && (h != 1600 || w != 1440)) {
    // two 1440 x 1600 eyes in a scratch of this entry point's own (grow-only): the context's warp-res planes belong to the render path, whose
    // slots may be in flight at another size (an ensure_work() here would shrink them under a queued pixel pass)
    const size_t ne = (size_t)1600 * 1440 * 3;
    if (c->fmt_cap < 2 * ne) { HIPCHK(re_alloc(&c->fmt_eyes, 2 * ne)); c->fmt_cap = 2 * ne; }
    vd_launch_resize_linear_u8(c->stream, left_bgr, h, w, c->fmt_eyes, 1600, 1440);
    vd_launch_resize_linear_u8(c->stream, right_bgr, h, w, c->fmt_eyes + ne, 1600, 1440);
    L = c->fmt_eyes; R = c->fmt_eyes + ne; eh = 1600; ew = 1440;
  }
  vd3d_render_params p;
  vd3d_render_params_default(&p);
  p.format = format; p.warp_w = ew; p.warp_h = eh; p.fit_w = ew; p.fit_h = eh;
  p.out_w = (format == VD3D_FMT_HALF_SBS || format == VD3D_FMT_FULL_SBS || format == VD3D_FMT_VR) ? 2 * ew : ew; p.out_h = eh;
  vd_finish_consts fc;
  memset(&fc, 0, sizeof fc);
  fc.sharp_kn = 0.f; fc.sharp_kc = 1.f;
  // identity fit: format_3d_output stacks / interleaves / mixes the eyes as they are (np.hstack, row slices, the anaglyph matrix) -- NOT the
  // render loop's pad_to_aspect_ratio, whose int(aspect * h) truncates to w - 1 for about one eye size in twenty (61x7, 1920x804, ...)
  vd_launch_sharp_mux(c->stream, L, R, p, fc, out_bgr, 0, true);
  HIPCHK(hipGetLastError());
  return 0;
}

// preprocess_esr / postprocess_esr / blend_images, core/merged_pipeline.py:219-236
VD3D_EXPORT int vd3d_esr_preprocess(vd3d_ctx* c, int dtype, const uint8_t* frame_bgr, long long pitch_bytes, int h, int w, int channels_last,
                                    void* out_rgb) {
  if (!c || !frame_bgr || !out_rgb || h < 1 || w < 1 || pitch_bytes < 3ll * w) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "esr_pre");
  if (!vd_launch_esr_pre(c->stream, dtype, frame_bgr, pitch_bytes, h, w, channels_last ? 1 : 0, out_rgb)) return set_err(VD3D_E_INVALID, "bad dtype %d", dtype);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_esr_postprocess(vd3d_ctx* c, const float* pred_rgb, int h, int w, int channels_last, int cy, int cx, int ch, int cw,
                                     uint8_t* out_bgr, long long pitch_bytes) {
  if (!c || !pred_rgb || !out_bgr || h < 1 || w < 1 || cy < 0 || cx < 0 || ch < 1 || cw < 1 || cy + ch > h || cx + cw > w || pitch_bytes < 3ll * cw)
    return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "esr_post");
  vd_launch_esr_post(c->stream, pred_rgb, h, w, channels_last ? 1 : 0, cy, cx, ch, cw, out_bgr, pitch_bytes);
  HIPCHK(hipGetLastError());
  return 0;
}

// run_rife's glue, core/merged_pipeline.py:195-218
VD3D_EXPORT int vd3d_rife_preprocess(vd3d_ctx* c, int dtype, const uint8_t* frame1_bgr, const uint8_t* frame2_bgr, int h, int w, int channels_last,
                                     void* out6) {
  if (!c || !frame1_bgr || !frame2_bgr || !out6 || h < 1 || w < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_rife_pre(c->stream, dtype, frame1_bgr, frame2_bgr, h, w, channels_last ? 1 : 0, out6)) return set_err(VD3D_E_INVALID, "bad dtype %d", dtype);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_rife_postprocess(vd3d_ctx* c, const float* pred3, int h, int w, int channels_last, uint8_t* out_bgr) {
  if (!c || !pred3 || !out_bgr || h < 1 || w < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  vd_launch_rife_post(c->stream, pred3, h, w, channels_last ? 1 : 0, out_bgr);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_add_weighted_u8(vd3d_ctx* c, const uint8_t* a, double alpha, const uint8_t* b, double beta, double gamma, long long n,
                                     uint8_t* out) {
  if (!c || !a || !b || !out || n < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "add_weighted");
  vd_launch_add_weighted_u8(c->stream, a, (float)alpha, b, (float)beta, (float)gamma, n, out);
  HIPCHK(hipGetLastError());
  return 0;
}

// a24: depth-net prediction [B][ph][pw] float32 -> uint8 depth planes [B][H][W] (bicubic post-process + per-frame min-max)
VD3D_EXPORT int vd3d_depth_handoff_form(vd3d_ctx* c, const float* pred, int B, int ph, int pw, int H, int W, int invert, uint8_t* out_gray, int form) {
  if (!c || !pred || !out_gray || B < 1 || ph < 1 || pw < 1 || H < 1 || W < 1) return set_err(VD3D_E_INVALID, "bad argument");
  if (form < 0 || form > 2) return set_err(VD3D_E_INVALID, "depth_handoff: form %d (0 = choose, 1 = general, 2 = separable)", form);
  HIPCHK(hipSetDevice(c->device));
  if (B > c->mm_cap) { HIPCHK(re_alloc(&c->mm, (size_t)3 * B)); c->mm_cap = B; }
  StageTimer t(c, "handoff");
  if (!vd_launch_depth_handoff(c->stream, pred, B, ph, pw, H, W, invert ? 1 : 0, c->mm, out_gray, form))
    return set_err(VD3D_E_UNSUPPORTED, "depth_handoff: the separable form is for up-scaling only (%dx%d -> %dx%d)", pw, ph, W, H);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_depth_handoff(vd3d_ctx* c, const float* pred, int B, int ph, int pw, int H, int W, int invert, uint8_t* out_gray) {
  return vd3d_depth_handoff_form(c, pred, B, ph, pw, H, W, invert, out_gray, 0);
}

// tiled high-resolution depth (vd3d_tiles.hip): infer_depth_tile's crops and blend, _normalize_to_u8 (core/render_depth.py:102-194)
VD3D_EXPORT int vd3d_tile_gather_cubic_u8(vd3d_ctx* c, const uint8_t* frames_bgr, long long pitch_bytes, long long frame_stride_bytes, int B, int H, int W,
                                          const int32_t* origins_dev, int n, int ch, int cw, int chs, int cws, uint8_t* out_tiles) {
  if (!c || !frames_bgr || !origins_dev || !out_tiles || B < 1 || H < 1 || W < 1 || n < 1 || ch < 1 || cw < 1 || chs < 1 || cws < 1)
    return set_err(VD3D_E_INVALID, "bad argument");
  if (ch > H || cw > W || pitch_bytes < 3ll * W || (B > 1 && frame_stride_bytes < pitch_bytes * H))
    return set_err(VD3D_E_INVALID, "tile_gather: crop %dx%d of a %dx%d frame, pitch %lld, frame stride %lld", cw, ch, W, H, pitch_bytes, frame_stride_bytes);
  if ((long long)n * chs * cws * 3 >= (1ll << 31)) return set_err(VD3D_E_INVALID, "tile batch too large");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "tile_gather");
  if (!vd_launch_tile_gather(c->stream, frames_bgr, pitch_bytes, frame_stride_bytes, B, H, W, origins_dev, n, ch, cw, chs, cws, out_tiles))
    return set_err(VD3D_E_UNSUPPORTED, "tile_gather: %d tiles in one launch (<= 65535)", n);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_tile_blend_f32(vd3d_ctx* c, const float* pred_pool, const int64_t* pred_off_dev, const int32_t* tile_tab_dev, const float* w_pool,
                                    int B, int tgt_h, int tgt_w, int tile, int pad, float* out) {
  if (!c || !pred_pool || !pred_off_dev || !tile_tab_dev || !w_pool || !out || B < 1 || B > 65535 || tgt_h < 1 || tgt_w < 1 || tile < 1 || pad < 0)
    return set_err(VD3D_E_INVALID, "bad argument");
  if ((reinterpret_cast<uintptr_t>(tile_tab_dev) & 15) != 0) return set_err(VD3D_E_INVALID, "tile_blend: the tile table must be 16-byte aligned");
  if ((long long)tgt_h * tgt_w >= (1ll << 31)) return set_err(VD3D_E_INVALID, "plane too large");
  const int core = tile - 2 * pad > 1 ? tile - 2 * pad : 1;
  if ((tile + core - 1) / core > 4)
    return set_err(VD3D_E_UNSUPPORTED, "tile_blend: tile %d with pad %d puts %d tiles over a pixel per axis (built for <= 4: pad <= 3/8 tile)", tile, pad,
                   (tile + core - 1) / core);
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "tile_blend");
  vd_launch_tile_blend(c->stream, pred_pool, reinterpret_cast<const long long*>(pred_off_dev), tile_tab_dev, w_pool, B, tgt_h, tgt_w, tile, core, out);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_depth_normalize_pclip_u8(vd3d_ctx* c, const float* planes, int B, int H, int W, float p_lo, float p_hi, int invert, uint8_t* out_gray,
                                              float* lo_hi_dev_or_null) {
  if (!c || !planes || !out_gray || B < 1 || B > 65535 || H < 1 || W < 1 || !(p_lo >= 0.f && p_lo <= p_hi && p_hi <= 100.f))
    return set_err(VD3D_E_INVALID, "bad argument");
  const long long n = (long long)H * W;
  if (n >= (1ll << 31)) return set_err(VD3D_E_INVALID, "plane too large");
  HIPCHK(hipSetDevice(c->device));
  if (B > c->pclip_cap) { HIPCHK(re_alloc(&c->pclip_ws, (size_t)B * VD_PCLIP_WS_WORDS)); c->pclip_cap = B; }
  // numpy.percentile, method "linear", on a float32 array: q = float32(p) / float32(100), virtual index = (n - 1) * q in float32, its floor and
  // the index after it, gamma = the fraction; at or beyond the last index both neighbours are the last element
  uint32_t rank[VD_PCLIP_NR];
  float g[2];
  const float pc[2] = {p_lo, p_hi};
  const float last = (float)(n - 1);
  for (int k = 0; k < 2; ++k) {
    const float q = pc[k] / 100.0f;
    const float vi = last * q;
    uint32_t k0, k1;
    if (vi >= last) { k0 = k1 = (uint32_t)(n - 1); g[k] = 0.f; }
    else { const float fl = floorf(vi); k0 = (uint32_t)fl; k1 = k0 + 1; g[k] = vi - fl; }
    if (k1 > (uint32_t)(n - 1)) k1 = (uint32_t)(n - 1);
    rank[1 + 2 * k] = k0; rank[2 + 2 * k] = k1;
  }
  rank[0] = 0; rank[5] = (uint32_t)(n - 1);
  StageTimer t(c, "pclip_u8");
  vd_launch_pclip_u8(c->stream, planes, B, n, rank, g[0], g[1], invert ? 1 : 0, c->pclip_ws, out_gray, lo_hi_dev_or_null);
  HIPCHK(hipGetLastError());
  return 0;
}

// letterbox handling of the depth pass (vd3d_letterbox.hip): LetterboxTracker and the bar fill (core/render_depth.py:280-573,1919-1933)
static int lb_check(vd3d_ctx* c, const void* p0, const void* p1, int B, int H, int W) {
  if (!c || !p0 || !p1 || B < 1 || H < 1 || W < 1) return set_err(VD3D_E_INVALID, "bad argument");
  if (!vd_lb_size_ok(B, H, W)) return set_err(VD3D_E_UNSUPPORTED, "letterbox: %d frames of %dx%d (built for W <= 8192, H <= 8192, B <= 4096)", B, W, H);
  return 0;
}

VD3D_EXPORT int vd3d_letterbox_stats(vd3d_ctx* c, const uint8_t* frames_bgr, int B, int H, int W, int chain, float* row_mean, float* row_var,
                                     uint32_t* row_sat_sum, uint8_t* gray, uint32_t* hist64, uint64_t* mad_sum, float* frame_mean) {
  if (!row_mean || !row_var || !row_sat_sum || !hist64 || !mad_sum || !frame_mean) return set_err(VD3D_E_INVALID, "bad argument");
  if (int rc = lb_check(c, frames_bgr, gray, B, H, W)) return rc;
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "letterbox_stats");
  HIPCHK(vd_lb_stats(&c->lb, c->stream, frames_bgr, B, H, W, chain ? 1 : 0, row_mean, row_var, row_sat_sum, gray, hist64,
                     reinterpret_cast<unsigned long long*>(mad_sum), frame_mean));
  if (chain) HIPCHK(vd_lb_stats_commit(&c->lb, c->stream, gray, hist64, B, H, W));
  return 0;
}

VD3D_EXPORT int vd3d_canny_u8(vd3d_ctx* c, const uint8_t* gray, int B, int H, int W, int low, int high, uint8_t* edges, int32_t* row_counts_or_null) {
  if (int rc = lb_check(c, gray, edges, B, H, W)) return rc;
  if (low < 0 || high < low || high > 1442) return set_err(VD3D_E_INVALID, "canny: thresholds %d, %d (0 <= low <= high <= 1442)", low, high);
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "canny");
  HIPCHK(vd_lb_canny(&c->lb, c->stream, gray, B, H, W, low, high, edges, row_counts_or_null));
  return 0;
}

VD3D_EXPORT int vd3d_canny_hysteresis_u8(vd3d_ctx* c, const uint8_t* classes, int B, int H, int W, uint8_t* edges, int32_t* row_counts_or_null) {
  if (int rc = lb_check(c, classes, edges, B, H, W)) return rc;
  if (classes == edges) return set_err(VD3D_E_INVALID, "canny_hysteresis: the edge map needs its own buffer");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "canny_hysteresis");
  HIPCHK(vd_lb_hysteresis(&c->lb, c->stream, classes, B, H, W, edges, row_counts_or_null));
  return 0;
}

VD3D_EXPORT int vd3d_letterbox_track(vd3d_ctx* c, const uint8_t* frames_bgr, int B, int H, int W, const vd3d_letterbox_params* params, int32_t* out_bars) {
  if (!params) return set_err(VD3D_E_INVALID, "bad argument");
  if (int rc = lb_check(c, frames_bgr, out_bars, B, H, W)) return rc;
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "letterbox_track");
  HIPCHK(vd_lb_track(&c->lb, c->stream, frames_bgr, B, H, W, params, out_bars));
  return 0;
}

VD3D_EXPORT int vd3d_letterbox_state_reset(vd3d_ctx* c) {
  if (!c) return set_err(VD3D_E_INVALID, "NULL context");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vd_lb_state_reset(&c->lb, c->stream));
  return 0;
}

VD3D_EXPORT int vd3d_letterbox_state_export(vd3d_ctx* c, vd3d_letterbox_state* out, uint32_t* prev_hist64_host_or_null, uint8_t* prev_gray_dev_or_null,
                                            long long gray_capacity) {
  if (!c || !out) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vd_lb_state_export(&c->lb, c->stream, out, prev_hist64_host_or_null, prev_gray_dev_or_null, gray_capacity));
  return 0;
}

VD3D_EXPORT int vd3d_letterbox_state_import(vd3d_ctx* c, const vd3d_letterbox_state* in, const uint32_t* prev_hist64_host_or_null,
                                            const uint8_t* prev_gray_dev_or_null) {
  if (!c || !in) return set_err(VD3D_E_INVALID, "bad argument");
  if (in->have_prev && prev_gray_dev_or_null && !vd_lb_size_ok(1, in->prev_h, in->prev_w)) return set_err(VD3D_E_INVALID, "letterbox state: previous frame %dx%d", in->prev_w, in->prev_h);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vd_lb_state_import(&c->lb, c->stream, in, prev_hist64_host_or_null, prev_gray_dev_or_null));
  return 0;
}

VD3D_EXPORT int vd3d_depth_letterbox_fill_u8(vd3d_ctx* c, const uint8_t* depth, int B, int H, int W, const int32_t* bars_dev, int bars_stride, uint8_t* out) {
  if (!bars_dev || bars_stride < 0 || bars_stride == 1) return set_err(VD3D_E_INVALID, "bad argument");
  if (int rc = lb_check(c, depth, out, B, H, W)) return rc;
  if (depth == out) return set_err(VD3D_E_INVALID, "depth_letterbox_fill: the output needs its own buffer");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "letterbox_fill");
  HIPCHK(vd_lb_fill(&c->lb, c->stream, depth, B, H, W, bars_dev, bars_stride, out));
  return 0;
}

VD3D_EXPORT int vd3d_depth_preprocess_form(vd3d_ctx* c, const uint8_t* frames_bgr, int B, int H, int W, int th, int tw,
                                           const float* mean3_host, const float* std3_host, int dtype, void* out_nhwc, int form) {
  if (form < 0 || form > 2) return set_err(VD3D_E_INVALID, "depth_preprocess: form %d (0 = choose, 1 = general, 2 = strip)", form);
  if (dtype != VD3D_DT_BF16 && dtype != VD3D_DT_F32) return set_err(VD3D_E_INVALID, "bad dtype %d", dtype);
  if (!c || !frames_bgr || !mean3_host || !std3_host || !out_nhwc || B < 1 || H < 1 || W < 1 || th < 1 || tw < 1)
    return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "depth_prep");
  const int rc = vd_launch_depth_prep(c->stream, frames_bgr, B, H, W, th, tw, mean3_host, std3_host, dtype, out_nhwc, form);
  if (rc == 1) return set_err(VD3D_E_UNSUPPORTED, "depth_preprocess: %dx%d -> %dx%d exceeds the antialias tap budget", W, H, tw, th);
  if (rc) return set_err(VD3D_E_UNSUPPORTED, "depth_preprocess: the strip form does not hold %dx%d -> %dx%d (down-scaling within its LDS plan only)", W, H, tw, th);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_depth_preprocess(vd3d_ctx* c, const uint8_t* frames_bgr, int B, int H, int W, int th, int tw,
                                      const float* mean3_host, const float* std3_host, int dtype, void* out_nhwc) {
  return vd3d_depth_preprocess_form(c, frames_bgr, B, H, W, th, tw, mean3_host, std3_host, dtype, out_nhwc, 0);
}

// ---- the Pillow-exact front end (vd3d_pilresample.hip) ------------------------------------------------------------------------------------------
// The context's table of one axis, built at its first use (std::list: an entry keeps its address).
static int pil_axis(vd3d_ctx* c, int n_in, int n_out, const vd_pil_axis** out) {
  for (const auto& a : c->pil_axes)
    if (a.n_in == n_in && a.n_out == n_out) { *out = &a; return 0; }
  vd_pil_axis a;
  hipError_t e = hipSuccess;
  if (vd_pil_axis_build(&a, n_in, n_out, &e) < 0) return set_err(VD3D_E_HIP, "pil tables %d -> %d: %s", n_in, n_out, hipGetErrorString(e));
  c->pil_axes.push_back(a);
  *out = &c->pil_axes.back();
  return 0;
}
// A context that has met more than 256 axes starts its list over, once nothing queued can read a table (tiled depth meets a handful per clip).
static int pil_axes_bound(vd3d_ctx* c) {
  if (c->pil_axes.size() <= 256) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& a : c->pil_axes) if (a.dev) (void)hipFree(a.dev);
  c->pil_axes.clear();
  return 0;
}
#define PIL_BUDGET_TEXT "exceeds the kernel's plan (24 taps per axis, 213 input pixels under 32 output columns, 65535 frames)"

VD3D_EXPORT int vd3d_resize_pil_bicubic_u8(vd3d_ctx* c, const uint8_t* src, int B, int H, int W, uint8_t* dst, int h, int w) {
  if (!c || !src || !dst) return set_err(VD3D_E_INVALID, "resize_pil_bicubic_u8: NULL argument");
  if (B < 1 || H < 1 || W < 1 || h < 1 || w < 1) return set_err(VD3D_E_INVALID, "resize_pil_bicubic_u8: %d frames of %dx%d -> %dx%d", B, W, H, w, h);
  HIPCHK(hipSetDevice(c->device));
  int rc = pil_axes_bound(c);
  if (rc) return rc;
  const vd_pil_axis *aw = nullptr, *ah = nullptr;
  if ((rc = pil_axis(c, W, w, &aw)) || (rc = pil_axis(c, H, h, &ah))) return rc;
  int by = 0;
  if (!vd_pil_plan(aw, ah, B, &by)) return set_err(VD3D_E_UNSUPPORTED, "resize_pil_bicubic_u8: %d x %dx%d -> %dx%d " PIL_BUDGET_TEXT, B, W, H, w, h);
  StageTimer t(c, "resize_pil");
  vd_launch_pil_resample(c->stream, src, B, H, W, aw, ah, 0, nullptr, dst);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_depth_preprocess_pil(vd3d_ctx* c, const uint8_t* frames_bgr, int B, int H, int W, int mid_h, int mid_w, int th, int tw,
                                          const float* mean3_host, const float* std3_host, int dtype, void* out_nhwc) {
  if (!c || !frames_bgr || !out_nhwc || !mean3_host || !std3_host) return set_err(VD3D_E_INVALID, "depth_preprocess_pil: NULL argument");
  if (B < 1 || H < 1 || W < 1 || th < 1 || tw < 1 || mid_h < 0 || mid_w < 0 || (mid_h > 0) != (mid_w > 0))
    return set_err(VD3D_E_INVALID, "depth_preprocess_pil: %d frames of %dx%d -> %dx%d -> %dx%d", B, W, H, mid_w, mid_h, tw, th);
  if (dtype != VD3D_DT_BF16 && dtype != VD3D_DT_F32) return set_err(VD3D_E_INVALID, "depth_preprocess_pil: dtype %d (float32 or bf16)", dtype);
  HIPCHK(hipSetDevice(c->device));
  int rc = pil_axes_bound(c);
  if (rc) return rc;
  const bool two = mid_h > 0;
  const int sh = two ? mid_h : H, sw = two ? mid_w : W;
  const vd_pil_axis *aw0 = nullptr, *ah0 = nullptr, *aw1 = nullptr, *ah1 = nullptr;
  if (two && ((rc = pil_axis(c, W, sw, &aw0)) || (rc = pil_axis(c, H, sh, &ah0)))) return rc;
  if ((rc = pil_axis(c, sw, tw, &aw1)) || (rc = pil_axis(c, sh, th, &ah1))) return rc;
  int by = 0;
  if ((two && !vd_pil_plan(aw0, ah0, B, &by)) || !vd_pil_plan(aw1, ah1, B, &by))
    return set_err(VD3D_E_UNSUPPORTED, "depth_preprocess_pil: %d x %dx%d -> %dx%d -> %dx%d " PIL_BUDGET_TEXT, B, W, H, sw, sh, tw, th);
  const float* lut = nullptr;
  for (const auto& t : c->pil_luts)
    if (!memcmp(t.mean, mean3_host, sizeof t.mean) && !memcmp(t.stdv, std3_host, sizeof t.stdv)) { lut = t.dev; break; }
  if (!lut) {
    if (c->pil_luts.size() >= 64) return set_err(VD3D_E_UNSUPPORTED, "depth_preprocess_pil: more than 64 (mean, std) pairs in one context");
    vd3d_ctx::pil_lut t;
    memcpy(t.mean, mean3_host, sizeof t.mean); memcpy(t.stdv, std3_host, sizeof t.stdv);
    float host[768];
    vd_pil_lut_fill(t.mean, t.stdv, host);
    HIPCHK(hipMalloc((void**)&t.dev, sizeof host));
    const hipError_t e = hipMemcpy(t.dev, host, sizeof host, hipMemcpyHostToDevice);   // blocking: there before any launch
    if (e != hipSuccess) { (void)hipFree(t.dev); return set_err(VD3D_E_HIP, "depth_preprocess_pil: table upload: %s", hipGetErrorString(e)); }
    c->pil_luts.push_back(t);
    lut = t.dev;
  }
  const uint8_t* src = frames_bgr;
  if (two) {
    const size_t need = (size_t)B * sh * sw * 3 + 4;   // and the dword the last row's last bytes are fetched in
    if (need > c->pil_mid_cap) { c->pil_mid_cap = 0; HIPCHK(re_alloc(&c->pil_mid, need)); c->pil_mid_cap = need; }   // hipFree waits for whatever still reads the old buffer
    StageTimer t(c, "depth_prep_pil");
    vd_launch_pil_resample(c->stream, frames_bgr, B, H, W, aw0, ah0, 0, nullptr, c->pil_mid);
    src = c->pil_mid;
  }
  {
    StageTimer t(c, "depth_prep_pil");
    vd_launch_pil_resample(c->stream, src, B, sh, sw, aw1, ah1, dtype == VD3D_DT_F32 ? 1 : 2, lut, out_nhwc);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_add_layernorm(vd3d_ctx* c, int dtype, const void* x, const void* y_or_null, const void* gamma, const void* beta,
                                   float eps, int64_t rows, int cols, void* out_sum, void* out_norm) {
  if (dtype != VD3D_DT_BF16 && dtype != VD3D_DT_F32) return set_err(VD3D_E_INVALID, "bad dtype %d", dtype);
  if (!c || !x || !gamma || !beta || !out_norm || rows < 1 || (y_or_null && !out_sum)) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_add_layernorm(c->stream, dtype, x, y_or_null, gamma, beta, eps, (long long)rows, cols, out_sum, out_norm))
    return set_err(VD3D_E_UNSUPPORTED, "add_layernorm: cols %d not in {384,768,1024}", cols);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int64_t vd3d_conv3x3_x2_weight_bytes(int Cin, int Cout) { return (int64_t)vd_conv3x3_x2_weight_bytes(Cin, Cout); }

VD3D_EXPORT int vd3d_conv3x3_x2_pack_weights(vd3d_ctx* c, const float* W, int Cin, int Cout, void* image) {
  if (!c || !W || !image) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_conv3x3_x2_pack(c->stream, W, Cin, Cout, image))
    return set_err(VD3D_E_UNSUPPORTED, "conv3x3_x2: C_in %d must be a positive multiple of 16 and C_out %d one of 64, 128", Cin, Cout);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_conv3x3_x2(vd3d_ctx* c, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y) {
  if (!c || !X || !w_image || !Y) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_conv3x3_x2(c->stream, X, B, H, W, Cin, w_image, Cout, Y))
    return set_err(VD3D_E_UNSUPPORTED, "conv3x3_x2: C_in %d (multiple of 16), C_out %d (64 | 128), B %d <= 65535, 16-byte aligned input and image", Cin, Cout, B);
  HIPCHK(hipGetLastError());
  return 0;
}

// the tile convolutions on dense, bias-free maps: one kernel body (vd3d_conv_x3.h) in two arithmetics and two strides, one checked entry point for all four.
// x3: bf16x3, stride 1 (vd3d_conv_x3.hip); s2_x3: its stride-2 form for the reassemble stage's wide maps (launch: vd3d_conv_s2.hip), C_out in multiples of 128;
// s1_x2 / s2_x2: the same two in the fp16x2 arithmetic (vd3d_conv_x2t.hip).
struct tile_conv_desc {
  const char* name;
  const char* cin_cap;    // the shape message's C_in bound, where weight_bytes has one
  const char* cout_rule;  // the shape message's C_out sentence
  long long (*weight_bytes)(int Cin, int Cout);
  bool (*pack)(hipStream_t s, const float* W, int Cin, int Cout, void* img);
  bool (*launch)(hipStream_t s, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, float* Y);
};
#define TILE_CONV(sfx, cap, rule) static const tile_conv_desc tc_##sfx = {"conv3x3_" #sfx, cap, rule, vd_conv3x3_##sfx##_weight_bytes, vd_launch_conv3x3_##sfx##_pack, vd_launch_conv3x3_##sfx}
TILE_CONV(x3, "", "one of 32, 64, 128, 256");
TILE_CONV(s2_x3, " (at most 65536)", "a positive multiple of 128 (at most 1024)");
TILE_CONV(s1_x2, " (at most 65536)", "one of 32, 64, 128, 256");
TILE_CONV(s2_x2, " (at most 65536)", "a positive multiple of 128 (at most 1024)");
#undef TILE_CONV

static int tile_conv_shape_err(const tile_conv_desc& d, int Cin, int Cout) {
  return set_err(VD3D_E_UNSUPPORTED, "%s: shape not built: C_in %d must be a positive multiple of 16%s and C_out %d %s", d.name, Cin, d.cin_cap, Cout, d.cout_rule);
}
static int tile_conv_pack(const tile_conv_desc& d, vd3d_ctx* c, const float* W, int Cin, int Cout, void* image) {
  if (!c || !W || !image) return set_err(VD3D_E_INVALID, "bad argument");
  if (d.weight_bytes(Cin, Cout) < 0) return tile_conv_shape_err(d, Cin, Cout);
  if (reinterpret_cast<uintptr_t>(image) & 15) return set_err(VD3D_E_UNSUPPORTED, "%s: the weight image must be 16-byte aligned", d.name);
  HIPCHK(hipSetDevice(c->device));
  if (!d.pack(c->stream, W, Cin, Cout, image)) return set_err(VD3D_E_HIP, "%s: the weight pack launch failed", d.name);
  HIPCHK(hipGetLastError());
  return 0;
}
static int tile_conv_run(const tile_conv_desc& d, vd3d_ctx* c, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y) {
  if (!c || !X || !w_image || !Y) return set_err(VD3D_E_INVALID, "bad argument");
  if (d.weight_bytes(Cin, Cout) < 0) return tile_conv_shape_err(d, Cin, Cout);
  if (B < 1 || B > 65535) return set_err(VD3D_E_UNSUPPORTED, "%s: batch %d must be 1 .. 65535 (one grid row per frame)", d.name, B);
  if (H < 1 || W < 1) return set_err(VD3D_E_UNSUPPORTED, "%s: map %d x %d must be at least 1 x 1", d.name, H, W);
  if ((reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(w_image) & 15) || (reinterpret_cast<uintptr_t>(Y) & 3))
    return set_err(VD3D_E_UNSUPPORTED, "%s: the input and the weight image must be 16-byte aligned (the output 4-byte)", d.name);
  HIPCHK(hipSetDevice(c->device));
  if (!d.launch(c->stream, X, B, H, W, Cin, w_image, Cout, Y)) return set_err(VD3D_E_HIP, "%s: the dynamic LDS opt-in or the launch failed", d.name);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int64_t vd3d_conv3x3_x3_weight_bytes(int Cin, int Cout) { return (int64_t)tc_x3.weight_bytes(Cin, Cout); }
VD3D_EXPORT int vd3d_conv3x3_x3_pack_weights(vd3d_ctx* c, const float* W, int Cin, int Cout, void* image) { return tile_conv_pack(tc_x3, c, W, Cin, Cout, image); }
VD3D_EXPORT int vd3d_conv3x3_x3(vd3d_ctx* c, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y) {
  return tile_conv_run(tc_x3, c, X, B, H, W, Cin, w_image, Cout, Y);
}
VD3D_EXPORT int64_t vd3d_conv3x3_s2_x3_weight_bytes(int Cin, int Cout) { return (int64_t)tc_s2_x3.weight_bytes(Cin, Cout); }
VD3D_EXPORT int vd3d_conv3x3_s2_x3_pack_weights(vd3d_ctx* c, const float* W, int Cin, int Cout, void* image) { return tile_conv_pack(tc_s2_x3, c, W, Cin, Cout, image); }
VD3D_EXPORT int vd3d_conv3x3_s2_x3(vd3d_ctx* c, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y) {
  return tile_conv_run(tc_s2_x3, c, X, B, H, W, Cin, w_image, Cout, Y);
}
VD3D_EXPORT int64_t vd3d_conv3x3_s1_x2_weight_bytes(int Cin, int Cout) { return (int64_t)tc_s1_x2.weight_bytes(Cin, Cout); }
VD3D_EXPORT int vd3d_conv3x3_s1_x2_pack_weights(vd3d_ctx* c, const float* W, int Cin, int Cout, void* image) { return tile_conv_pack(tc_s1_x2, c, W, Cin, Cout, image); }
VD3D_EXPORT int vd3d_conv3x3_s1_x2(vd3d_ctx* c, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y) {
  return tile_conv_run(tc_s1_x2, c, X, B, H, W, Cin, w_image, Cout, Y);
}
VD3D_EXPORT int64_t vd3d_conv3x3_s2_x2_weight_bytes(int Cin, int Cout) { return (int64_t)tc_s2_x2.weight_bytes(Cin, Cout); }
VD3D_EXPORT int vd3d_conv3x3_s2_x2_pack_weights(vd3d_ctx* c, const float* W, int Cin, int Cout, void* image) { return tile_conv_pack(tc_s2_x2, c, W, Cin, Cout, image); }
VD3D_EXPORT int vd3d_conv3x3_s2_x2(vd3d_ctx* c, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, float* Y) {
  return tile_conv_run(tc_s2_x2, c, X, B, H, W, Cin, w_image, Cout, Y);
}

// the stride-1 tile convolution with a residual unit's glue in its epilogue (vd3d_conv_epi.hip), on the weight image of the mode's bias-free entry point
VD3D_EXPORT int vd3d_conv3x3_epi(vd3d_ctx* c, int mode, const float* X, int B, int H, int W, int Cin, const void* w_image, int Cout, int flags,
                                 const float* bias_or_null, const float* r1_or_null, const float* r2_or_null, float* Y, float* Yrelu_or_null) {
  if (!c || !X || !w_image || !Y) return set_err(VD3D_E_INVALID, "conv3x3_epi: null argument");
  if (mode != VD3D_X3_BF16X3 && mode != VD3D_X3_FP16X2) return set_err(VD3D_E_INVALID, "conv3x3_epi: mode %d must be VD3D_X3_BF16X3 (0) or VD3D_X3_FP16X2 (1)", mode);
  if (flags & ~(VD3D_EPI_RELU_IN | VD3D_EPI_RELU)) return set_err(VD3D_E_INVALID, "conv3x3_epi: flags %d hold a bit that is neither VD3D_EPI_RELU_IN nor VD3D_EPI_RELU", flags);
  const tile_conv_desc& d = mode == VD3D_X3_BF16X3 ? tc_x3 : tc_s1_x2;
  if (d.weight_bytes(Cin, Cout) < 0)
    return set_err(VD3D_E_UNSUPPORTED, "conv3x3_epi: shape not built: C_in %d must be a positive multiple of 16%s and C_out %d %s", Cin, d.cin_cap, Cout, d.cout_rule);
  if (B < 1 || B > 65535) return set_err(VD3D_E_UNSUPPORTED, "conv3x3_epi: batch %d must be 1 .. 65535 (one grid row per frame)", B);
  if (H < 1 || W < 1) return set_err(VD3D_E_UNSUPPORTED, "conv3x3_epi: map %d x %d must be at least 1 x 1", H, W);
  HIPCHK(hipSetDevice(c->device));
  const int rc = vd_launch_conv3x3_epi(c->stream, mode == VD3D_X3_BF16X3 ? 0 : 1, X, B, H, W, Cin, w_image, Cout, flags, bias_or_null, r1_or_null, r2_or_null, Y, Yrelu_or_null);
  if (rc == 1 || rc == 2) return set_err(VD3D_E_UNSUPPORTED, "conv3x3_epi: the input and the weight image must be 16-byte aligned (bias, r1, r2 and the outputs 4-byte)");
  if (rc == 3) return set_err(VD3D_E_UNSUPPORTED, "conv3x3_epi: an output overlaps X, r1, r2, the bias, the weight image or the other output (a workgroup reads the halo of its neighbours' tiles)");
  if (rc) return set_err(VD3D_E_HIP, "conv3x3_epi: the dynamic LDS opt-in or the launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}

// DepthPro's head behind head.layers.0 (vd3d_depthpro_head.hip): every rule of include/vd3d.h is checked here, before anything is launched
static int depthpro_head_shape_err(int mode, int Cin) {
  if (mode != VD3D_X3_BF16X3 && mode != VD3D_X3_FP16X2) return set_err(VD3D_E_INVALID, "depthpro_head: mode %d must be VD3D_X3_BF16X3 (0) or VD3D_X3_FP16X2 (1)", mode);
  return set_err(VD3D_E_UNSUPPORTED, "depthpro_head: shape not built: C_in %d must be a positive multiple of 16 (at most 65536); C_out is 32", Cin);
}
VD3D_EXPORT int64_t vd3d_depthpro_head_weight_bytes(int mode, int Cin) { return (int64_t)vd_depthpro_head_weight_bytes(mode, Cin); }
VD3D_EXPORT int vd3d_depthpro_head_pack_weights(vd3d_ctx* c, int mode, const float* Wc, int Cin, void* image) {
  if (!c || !Wc || !image) return set_err(VD3D_E_INVALID, "depthpro_head: null argument");
  if (vd_depthpro_head_weight_bytes(mode, Cin) < 0) return depthpro_head_shape_err(mode, Cin);
  if ((reinterpret_cast<uintptr_t>(image) & 15) || (reinterpret_cast<uintptr_t>(Wc) & 3)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_head: the weight image must be 16-byte aligned (the blocks 4-byte)");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_depthpro_head_pack(c->stream, mode, Wc, Cin, image)) return set_err(VD3D_E_HIP, "depthpro_head: the weight pack launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_depthpro_head(vd3d_ctx* c, int mode, const float* x, int B, int h, int w, int Cin, const void* w_image, const float* T, const float* w3, float b3,
                                   float* out) {
  if (!c || !x || !w_image || !T || !w3 || !out) return set_err(VD3D_E_INVALID, "depthpro_head: null argument");
  if (vd_depthpro_head_weight_bytes(mode, Cin) < 0) return depthpro_head_shape_err(mode, Cin);
  if (B < 1 || B > 65535) return set_err(VD3D_E_UNSUPPORTED, "depthpro_head: batch %d must be 1 .. 65535 (one grid row per frame)", B);
  if (h < 1 || w < 1 || h > (1 << 14) || w > (1 << 14)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_head: coarse map %d x %d must be 1 x 1 .. 16384 x 16384", h, w);
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(w_image) & 15) || (reinterpret_cast<uintptr_t>(T) & 3) || (reinterpret_cast<uintptr_t>(w3) & 3) ||
      (reinterpret_cast<uintptr_t>(out) & 3))
    return set_err(VD3D_E_UNSUPPORTED, "depthpro_head: the input and the weight image must be 16-byte aligned (T, w3 and the output 4-byte)");
  {
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
    const uintptr_t xn = (uintptr_t)B * h * w * Cin * 4, on = (uintptr_t)B * h * w * 16;
    if (xa < oa + on && oa < xa + xn) return set_err(VD3D_E_UNSUPPORTED, "depthpro_head: the output overlaps the input (a workgroup reads the halo of its neighbours' tiles)");
  }
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_depthpro_head(c->stream, mode, x, B, h, w, Cin, w_image, T, w3, b3, out)) return set_err(VD3D_E_HIP, "depthpro_head: the dynamic LDS opt-in or the launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}

// the convolutions of the interpolation network (vd3d_conv_ifn.hip): every rule of include/vd3d.h is checked here, before anything is launched
VD3D_EXPORT int64_t vd3d_conv_ifn_weight_bytes(int kind, int Cin, int Cout) { return (int64_t)vd_conv_ifn_weight_bytes(kind, Cin, Cout); }

static int conv_ifn_shape_err(int kind, int Cin, int Cout) {
  return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: shape not built: kind %d must be 0 (3x3 s1), 1 (3x3 s2) or 2 (transposed 4x4 s2), C_in %d a positive multiple of 16 and C_out %d one of 32, 64, 96",
                 kind, Cin, Cout);
}

VD3D_EXPORT int vd3d_conv_ifn_pack_weights(vd3d_ctx* c, int kind, const float* W, int Cin, int Cout, void* image) {
  if (!c || !W || !image) return set_err(VD3D_E_INVALID, "conv_ifn: null argument");
  if (vd_conv_ifn_weight_bytes(kind, Cin, Cout) < 0) return conv_ifn_shape_err(kind, Cin, Cout);
  if ((reinterpret_cast<uintptr_t>(image) & 15) || (reinterpret_cast<uintptr_t>(W) & 3)) return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: the weight image must be 16-byte aligned (the weight 4-byte)");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_conv_ifn_pack(c->stream, kind, W, Cin, Cout, image)) return set_err(VD3D_E_HIP, "conv_ifn: the weight pack launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_conv_ifn(vd3d_ctx* c, int kind, const float* X, int B, int H, int W, int x_stride, int Cin, const void* w_image, const float* bias,
                              const float* slope_or_null, int Cout, const float* r_or_null, int r_stride, float* Y, int y_stride, int y_offset) {
  if (!c || !X || !w_image || !bias || !Y) return set_err(VD3D_E_INVALID, "conv_ifn: null argument");
  if (vd_conv_ifn_weight_bytes(kind, Cin, Cout) < 0) return conv_ifn_shape_err(kind, Cin, Cout);
  if (B < 1 || B > 65535) return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: batch %d must be 1 .. 65535 (one grid row per frame)", B);
  if (H < 1 || W < 1 || H > 32768 || W > 32768) return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: map %d x %d must be 1 .. 32768 on each side", H, W);
  if (x_stride < Cin || (x_stride & 3)) return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: x_stride %d must be a multiple of 4 and >= C_in %d", x_stride, Cin);
  if (y_offset < 0 || y_stride < y_offset + Cout)
    return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: y_offset %d must be >= 0 and y_offset + C_out %d <= y_stride %d", y_offset, Cout, y_stride);
  if (r_or_null && r_stride < Cout) return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: the residual's r_stride %d must be >= C_out %d", r_stride, Cout);
  if (((uintptr_t)X | (uintptr_t)w_image) & 15) return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: the input and the weight image must be 16-byte aligned");
  if (((uintptr_t)bias | (uintptr_t)slope_or_null | (uintptr_t)r_or_null | (uintptr_t)Y) & 3)
    return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: bias, slope, residual and output must be 4-byte aligned");
  const int Ho = kind == VD3D_IFN_K3S2 ? (H + 1) / 2 : kind == VD3D_IFN_T4S2 ? 2 * H : H, Wo = kind == VD3D_IFN_K3S2 ? (W + 1) / 2 : kind == VD3D_IFN_T4S2 ? 2 * W : W;
  {   // the bytes read (channels [0, C_in) of every input pixel) and the bytes written (the output slice of every pixel) must not meet
    const long long in_pix = (long long)B * H * W, out_pix = (long long)B * Ho * Wo;
    const uintptr_t xb = (uintptr_t)X, xe = xb + (uintptr_t)(((in_pix - 1) * x_stride + Cin) * 4);
    const uintptr_t yb = (uintptr_t)Y + (uintptr_t)y_offset * 4, ye = (uintptr_t)Y + (uintptr_t)(((out_pix - 1) * y_stride + y_offset + Cout) * 4);
    const bool same_grid = (const void*)X == (const void*)Y && x_stride == y_stride && kind == VD3D_IFN_K3S1;
    if (same_grid ? y_offset < Cin : (xb < ye && yb < xe))
      return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: the output slice [%d, %d) meets the input channels [0, %d) of the same buffer (a race between workgroups)",
                     y_offset, y_offset + Cout, Cin);
    if (r_or_null) {
      const uintptr_t rb = (uintptr_t)r_or_null, re = rb + (uintptr_t)(((out_pix - 1) * r_stride + Cout) * 4);
      const bool rgrid = (const void*)r_or_null == (const void*)Y && r_stride == y_stride;
      if (rgrid ? y_offset < Cout : (rb < ye && yb < re)) return set_err(VD3D_E_UNSUPPORTED, "conv_ifn: the residual overlaps the output slice");
    }
  }
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "conv_ifn");
  if (!vd_launch_conv_ifn(c->stream, kind, X, B, H, W, x_stride, Cin, w_image, bias, slope_or_null, Cout, r_or_null, r_stride, Y, y_stride, y_offset))
    return set_err(VD3D_E_HIP, "conv_ifn: the dynamic LDS opt-in failed");
  HIPCHK(hipGetLastError());
  return 0;
}

static int rife_glue_err(const char* what, int N, int h, int w, int scale) {
  return set_err(VD3D_E_UNSUPPORTED, "%s: N %d must be 1 .. 65535, the frame %d x %d 1 .. 32768 on each side, scale %d one of 1, 2, 4 and every pointer 16-byte aligned", what, N, h, w, scale);
}
static bool rife_glue_ok(int N, int h, int w, int scale) { return N >= 1 && N <= 65535 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768 && (scale == 1 || scale == 2 || scale == 4); }

VD3D_EXPORT int vd3d_rife_warp_pack(vd3d_ctx* c, const float* x6, const float* state_or_null, int N, int h, int w, int scale, float* out16) {
  if (!c || !x6 || !out16) return set_err(VD3D_E_INVALID, "rife_warp_pack: null argument");
  if (!rife_glue_ok(N, h, w, scale) || (((uintptr_t)x6 | (uintptr_t)state_or_null | (uintptr_t)out16) & 15)) return rife_glue_err("rife_warp_pack", N, h, w, scale);
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "rife_glue");
  vd_launch_rife_warp_pack(c->stream, x6, state_or_null, state_or_null ? 0 : 1, N, h, w, (h + 31) / 32 * 32, (w + 31) / 32 * 32, scale, out16);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_rife_update(vd3d_ctx* c, const float* t_, int t_stride, int first, int N, int h, int w, int scale, float* state) {
  if (!c || !t_ || !state) return set_err(VD3D_E_INVALID, "rife_update: null argument");
  if (!rife_glue_ok(N, h, w, scale) || (((uintptr_t)t_ | (uintptr_t)state) & 15)) return rife_glue_err("rife_update", N, h, w, scale);
  if (t_stride < 5 || (t_stride & 3)) return set_err(VD3D_E_UNSUPPORTED, "rife_update: t_stride %d must be a multiple of 4 and >= 5", t_stride);
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "rife_glue");
  vd_launch_rife_update(c->stream, t_, t_stride, first ? 1 : 0, N, (h + 31) / 32 * 32, (w + 31) / 32 * 32, scale, state);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_rife_blend(vd3d_ctx* c, const float* x6, const float* state, int N, int h, int w, float* out) {
  if (!c || !x6 || !state || !out) return set_err(VD3D_E_INVALID, "rife_blend: null argument");
  if (!rife_glue_ok(N, h, w, 1) || (((uintptr_t)x6 | (uintptr_t)state | (uintptr_t)out) & 15)) return rife_glue_err("rife_blend", N, h, w, 1);
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "rife_glue");
  vd_launch_rife_blend(c->stream, x6, state, N, h, w, (h + 31) / 32 * 32, (w + 31) / 32 * 32, out);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int64_t vd3d_attention_x3_workspace_bytes(int B, int T, int H, int D, int mode) { return (int64_t)vd_attn_x3_workspace_bytes(B, T, H, D, mode); }

VD3D_EXPORT int vd3d_attention_x3(vd3d_ctx* c, const float* qkv, int B, int T, int H, int D, float scale, int mode, void* workspace, int64_t workspace_bytes, float* out) {
  if (!c || !qkv || !workspace || !out) return set_err(VD3D_E_INVALID, "bad argument");
  const long long need = vd_attn_x3_workspace_bytes(B, T, H, D, mode);
  if (need < 0) return set_err(VD3D_E_UNSUPPORTED, "attention_x3: head size %d not built (64), an unknown mode %d or an empty shape (B %d T %d H %d)", D, mode, B, T, H);
  if (workspace_bytes < need) return set_err(VD3D_E_INVALID, "attention_x3: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, need);
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_attn_x3(c->stream, qkv, B, T, H, D, scale, workspace, out, mode))
    return set_err(VD3D_E_UNSUPPORTED, "attention_x3: qkv / workspace / out must be 16-byte aligned, B * H <= 65535");
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_attention_f32_form(vd3d_ctx* c, const float* qkv, int B, int T, int H, int D, float scale, float* out, int form) {
  if (!c || !qkv || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (form != 0 && form != 4 && form != 8) return set_err(VD3D_E_INVALID, "attention_f32: form %d is not 0 (choose), 4 or 8 waves per workgroup", form);
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_attn_f32(c->stream, qkv, B, T, H, D, scale, out, form))
    return set_err(VD3D_E_UNSUPPORTED, "attention_f32: head size %d not built (64), an empty shape (B %d T %d H %d), B * H > 65535 or qkv / out not 16-byte aligned", D, B, T, H);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_attention_f32(vd3d_ctx* c, const float* qkv, int B, int T, int H, int D, float scale, float* out) {
  return vd3d_attention_f32_form(c, qkv, B, T, H, D, scale, out, 0);
}

VD3D_EXPORT int64_t vd3d_gemm_x3_weight_bytes(int N, int K, int mode) { return (int64_t)vd_gemm_x3_weight_bytes(N, K, mode); }

VD3D_EXPORT int vd3d_gemm_x3_pack_weights(vd3d_ctx* c, const float* W, int N, int K, int mode, void* image) {
  if (!c || !W || !image) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_gemm_x3_pack_w(c->stream, W, N, K, image, mode)) return set_err(VD3D_E_UNSUPPORTED, "gemm_x3: K %d must be a positive multiple of 16 (N %d), mode %d in {0, 1}", K, N, mode);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_gemm_x3(vd3d_ctx* c, const float* X, int64_t M, int K, const void* w_image, int N, int mode, const float* bias_or_null, int epilogue, float* Y) {
  if (!c || !X || !w_image || !Y || M < 1) return set_err(VD3D_E_INVALID, "bad argument");
  if (epilogue != VD3D_GEMM_EPI_NONE && epilogue != VD3D_GEMM_EPI_GELU) return set_err(VD3D_E_INVALID, "gemm_x3: unknown epilogue %d", epilogue);
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_gemm_x3(c->stream, X, (long long)M, K, w_image, N, bias_or_null, epilogue, Y, mode))
    return set_err(VD3D_E_UNSUPPORTED, "gemm_x3: K %d must be a positive multiple of 16, mode %d in {0, 1}, X and the weight image 16-byte aligned", K, mode);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_upsample_bilinear_nhwc(vd3d_ctx* c, int dtype, const void* in, void* out, int B, int ih, int iw, int oh, int ow, int C) {
  if (dtype != VD3D_DT_BF16 && dtype != VD3D_DT_F32) return set_err(VD3D_E_INVALID, "bad dtype %d", dtype);
  if (!c || !in || !out || B < 1 || ih < 1 || iw < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_upsample_bilinear_nhwc(c->stream, dtype, in, out, B, ih, iw, oh, ow, C))
    return set_err(VD3D_E_UNSUPPORTED, "upsample_bilinear_nhwc: C not a multiple of 8 (bf16) / 4 (f32) or output smaller than 2x2");
  HIPCHK(hipGetLastError());
  return 0;
}

// DPT neck / head glue in float32 (vd3d_netops.hip): NHWC maps of n_pix pixels x C channels
VD3D_EXPORT int vd3d_nhwc_bias_act_f32(vd3d_ctx* c, const float* y, const float* bias_or_null, const float* r1_or_null, const float* r2_or_null, int relu,
                                       int64_t n_pix, int C, float* out, float* relu_out_or_null) {
  if (!c || !y || !out || n_pix < 1 || C < 4) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_bias_act_f32(c->stream, y, bias_or_null, r1_or_null, r2_or_null, relu, (long long)n_pix, C, out, relu_out_or_null))
    return set_err(VD3D_E_UNSUPPORTED, "nhwc_bias_act: C %d not a multiple of 4", C);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_upsample_bilinear_bias_nhwc_f32(vd3d_ctx* c, const float* in, const float* bias, float* out, int B, int ih, int iw, int oh, int ow, int C) {
  if (!c || !in || !bias || !out || B < 1 || ih < 1 || iw < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_upsample_bilinear_bias_nhwc_f32(c->stream, in, bias, out, B, ih, iw, oh, ow, C))
    return set_err(VD3D_E_UNSUPPORTED, "upsample_bilinear_bias_nhwc: C not a multiple of 4 or output smaller than 2x2");
  HIPCHK(hipGetLastError());
  return 0;
}
// one body for both entry points: the checks, in this order, are the same whatever the activation
static int dpt_head_tail(vd3d_ctx* c, const float* y, const float* b2, const float* w3, float b3, float scale, int64_t n_pix, int C, int act, float* out) {
  if (!c || !y || !b2 || !w3 || !out || n_pix < 1) return set_err(VD3D_E_INVALID, "bad argument");
  if (act != VD3D_HEAD_ACT_RELU && act != VD3D_HEAD_ACT_SIGMOID) return set_err(VD3D_E_INVALID, "dpt_head_tail: unknown activation %d", act);
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_head_tail_f32(c->stream, y, b2, w3, b3, scale, (long long)n_pix, C, act, out))
    return set_err(VD3D_E_UNSUPPORTED, "dpt_head_tail: C %d not in {16, 32, 64}, or y / b2 / w3 not 16-byte aligned", C);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_dpt_head_tail_f32(vd3d_ctx* c, const float* y, const float* b2, const float* w3, float b3, float scale, int64_t n_pix, int C, float* out) {
  return dpt_head_tail(c, y, b2, w3, b3, scale, n_pix, C, VD3D_HEAD_ACT_RELU, out);
}
VD3D_EXPORT int vd3d_dpt_head_tail_act_f32(vd3d_ctx* c, const float* y, const float* b2, const float* w3, float b3, float scale, int64_t n_pix, int C, int act,
                                           float* out) {
  return dpt_head_tail(c, y, b2, w3, b3, scale, n_pix, C, act, out);
}
VD3D_EXPORT int64_t vd3d_dpt_head_conv_weight_bytes(int Cin, int Cout) { return (int64_t)vd_dpt_head_conv_weight_bytes(Cin, Cout); }
VD3D_EXPORT int vd3d_dpt_head_conv_pack_weights(vd3d_ctx* c, const float* W, int Cin, int Cout, void* image) {
  if (!c || !W || !image) return set_err(VD3D_E_INVALID, "bad argument");
  if (vd_dpt_head_conv_weight_bytes(Cin, Cout) < 0)
    return set_err(VD3D_E_UNSUPPORTED, "dpt_head_conv: shape not built: %d -> %d channels (built: 32 | 64 | 128 -> 32 with the tail, 128 -> 64 plain)", Cin, Cout);
  if (reinterpret_cast<uintptr_t>(image) & 15) return set_err(VD3D_E_UNSUPPORTED, "dpt_head_conv: the weight image must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_dpt_head_conv_pack(c->stream, W, Cin, Cout, image)) return set_err(VD3D_E_HIP, "dpt_head_conv: the weight pack launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_dpt_head_conv_f32(vd3d_ctx* c, const float* x, const float* b_in, int B, int ih, int iw, int oh, int ow, int Cin, const void* w_image, int Cout,
                                       const float* b2_or_null, const float* w3_or_null, float b3, float scale, float* out) {
  if (!c || !x || !b_in || !w_image || !out || (b2_or_null == nullptr) != (w3_or_null == nullptr)) return set_err(VD3D_E_INVALID, "bad argument");
  const bool tail = b2_or_null != nullptr;
  if (!vd_dpt_head_conv_shape_ok(B, ih, iw, oh, ow, Cin, Cout, tail))
    return set_err(VD3D_E_UNSUPPORTED, "dpt_head_conv: shape not built: %d -> %d channels %s, batch %d, %d x %d -> %d x %d (built: 32 | 64 | 128 -> 32 with the tail, "
                   "128 -> 64 plain; batch 1 .. 65535; output at least 2 x 2; a frame below 2^31 elements)", Cin, Cout, tail ? "with the tail" : "plain", B, ih, iw, oh, ow);
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(b_in) & 15) || (reinterpret_cast<uintptr_t>(w_image) & 15) ||
      (reinterpret_cast<uintptr_t>(out) & (tail ? 3 : 15)) || (tail && ((reinterpret_cast<uintptr_t>(b2_or_null) & 15) || (reinterpret_cast<uintptr_t>(w3_or_null) & 15))))
    return set_err(VD3D_E_UNSUPPORTED, "dpt_head_conv: x, b_in, the weight image, b2, w3 and a plain output must be 16-byte aligned (the tail's output 4-byte)");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_dpt_head_conv_f32(c->stream, x, b_in, B, ih, iw, oh, ow, Cin, w_image, Cout, b2_or_null, w3_or_null, b3, scale, out))
    return set_err(VD3D_E_HIP, "dpt_head_conv: the dynamic LDS opt-in or the launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int64_t vd3d_neck_poly_weight_bytes(int Cin, int Cout, int f) { return (int64_t)vd_neck_poly_weight_bytes(Cin, Cout, f); }
VD3D_EXPORT int vd3d_neck_poly_pack_f32(vd3d_ctx* c, const float* Wc, int Cin, int Cout, int f, void* image) {
  if (!c || !Wc || !image) return set_err(VD3D_E_INVALID, "bad argument");
  if (vd_neck_poly_weight_bytes(Cin, Cout, f) < 0)
    return set_err(VD3D_E_UNSUPPORTED, "neck_poly: shape not built: %d -> %d channels, factor %d (built: 96 -> 128 and 48 -> 64 with factor 4, 192 -> 128 and 96 -> 64 with factor 2)",
                   Cin, Cout, f);
  if ((reinterpret_cast<uintptr_t>(image) & 15) || (reinterpret_cast<uintptr_t>(Wc) & 15))
    return set_err(VD3D_E_UNSUPPORTED, "neck_poly: the composed weights and the weight image must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_neck_poly_pack(c->stream, Wc, Cin, Cout, f, image)) return set_err(VD3D_E_HIP, "neck_poly: the weight pack launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_neck_poly_conv_f32(vd3d_ctx* c, const float* x, int B, int h, int w, int Cin, const void* w_image, const float* bc, int Cout, int f, float* out) {
  if (!c || !x || !w_image || !bc || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (!vd_neck_poly_shape_ok(B, h, w, Cin, Cout, f))
    return set_err(VD3D_E_UNSUPPORTED, "neck_poly: shape not built: %d -> %d channels, factor %d, batch %d, %d x %d (built: 96 -> 128 and 48 -> 64 with factor 4, 192 -> 128 and "
                   "96 -> 64 with factor 2; a batch's fine map below 2^31 pixels, its coarse map below 2^31 elements)", Cin, Cout, f, B, h, w);
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(w_image) & 15) || (reinterpret_cast<uintptr_t>(bc) & 15) || (reinterpret_cast<uintptr_t>(out) & 15))
    return set_err(VD3D_E_UNSUPPORTED, "neck_poly: x, the weight image, the bias blocks and the output must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_neck_poly_conv_f32(c->stream, x, B, h, w, Cin, w_image, bc, Cout, f, out)) return set_err(VD3D_E_HIP, "neck_poly: the launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_head_upconv_gather_f32(vd3d_ctx* c, const float* z, int B, int h, int w, int H, int W, int Cout, float* out) {
  // the shape first: a refusal needs neither a context nor a device
  if (!vd_head_upconv_shape_ok(B, h, w, H, W, Cout))
    return set_err(VD3D_E_UNSUPPORTED, "head_upconv: shape not built: %d output channels, batch %d, %d x %d -> %d x %d (built: 64 and 32 channels; an output of at least "
                   "2 x 2; a coarse row below 2^31 elements; a down-sampling factor of at most about 9)", Cout, B, h, w, H, W);
  if (!c || !z || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if ((reinterpret_cast<uintptr_t>(z) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return set_err(VD3D_E_UNSUPPORTED, "head_upconv: Z and the output must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_head_upconv_gather_f32(c->stream, z, B, h, w, H, W, Cout, out)) return set_err(VD3D_E_HIP, "head_upconv: the launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int64_t vd3d_head_conv_gather_weight_bytes(int Cin) { return (int64_t)vd_head_conv_gather_weight_bytes(Cin); }
VD3D_EXPORT int vd3d_head_conv_gather_tile(int ih, int iw, int oh, int ow, int Cin, int* th, int* tw) {
  if (!vd_head_conv_gather_shape_ok(1, ih, iw, oh, ow, Cin, th, tw))
    return set_err(VD3D_E_UNSUPPORTED, "head_conv_gather: shape not built: %d input channels, %d x %d -> %d x %d (built: 32 | 64 | 128 channels; an output of at least 2 x 2; "
                   "a down-sampling factor of at most about 6)", Cin, ih, iw, oh, ow);
  return 0;
}
VD3D_EXPORT int vd3d_head_conv_gather_pack_weights(vd3d_ctx* c, const float* Wt, int Cin, void* image) {
  if (vd_head_conv_gather_weight_bytes(Cin) < 0)
    return set_err(VD3D_E_UNSUPPORTED, "head_conv_gather: shape not built: %d input channels (built: 32 | 64 | 128 -> 32 with the tail)", Cin);
  if (!c || !Wt || !image) return set_err(VD3D_E_INVALID, "bad argument");
  if ((reinterpret_cast<uintptr_t>(image) & 15) || (reinterpret_cast<uintptr_t>(Wt) & 15))
    return set_err(VD3D_E_UNSUPPORTED, "head_conv_gather: the composed weights and the weight image must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_head_conv_gather_pack(c->stream, Wt, Cin, image)) return set_err(VD3D_E_HIP, "head_conv_gather: the weight pack launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_head_conv_gather_f32(vd3d_ctx* c, const float* y1, int B, int ih, int iw, int oh, int ow, int Cin, const void* w_image, const float* bc,
                                          const float* b2, const float* w3, float b3, float scale, float* out) {
  // the shape first: a refusal needs neither a context nor a device
  if (!vd_head_conv_gather_shape_ok(B, ih, iw, oh, ow, Cin, nullptr, nullptr))
    return set_err(VD3D_E_UNSUPPORTED, "head_conv_gather: shape not built: %d input channels, batch %d, %d x %d -> %d x %d (built: 32 | 64 | 128 -> 32 with the tail; an output of "
                   "at least 2 x 2; a coarse row below 2^31 elements; a down-sampling factor of at most about 6)", Cin, B, ih, iw, oh, ow);
  if (!c || !y1 || !w_image || !bc || !b2 || !w3 || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if ((reinterpret_cast<uintptr_t>(y1) & 15) || (reinterpret_cast<uintptr_t>(w_image) & 15) || (reinterpret_cast<uintptr_t>(bc) & 15) || (reinterpret_cast<uintptr_t>(b2) & 15) ||
      (reinterpret_cast<uintptr_t>(w3) & 15) || (reinterpret_cast<uintptr_t>(out) & 3))
    return set_err(VD3D_E_UNSUPPORTED, "head_conv_gather: y1, the weight image, bc, b2 and w3 must be 16-byte aligned (the output 4-byte)");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_head_conv_gather_f32(c->stream, y1, B, ih, iw, oh, ow, Cin, w_image, bc, b2, w3, b3, scale, out))
    return set_err(VD3D_E_HIP, "head_conv_gather: the dynamic LDS opt-in or the launch failed");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_depth_to_space_bias_nhwc_f32(vd3d_ctx* c, const float* y, const float* bias_or_null, int B, int H, int W, int s, int C, float* out) {
  if (!c || !y || !out || B < 1 || H < 1 || W < 1 || s < 1 || C < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_depth_to_space_bias_f32(c->stream, y, bias_or_null, B, H, W, s, C, out))
    return set_err(VD3D_E_UNSUPPORTED, "depth_to_space_bias: C %d not a multiple of 4, y / bias / out not 16-byte aligned, or a map too large for one grid", C);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_patchify_f32(vd3d_ctx* c, const float* x, int B, int th, int tw, int p, float* out) {
  if (!c || !x || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (B < 1 || p < 1 || p > 64 || th < p || tw < p)
    return set_err(VD3D_E_UNSUPPORTED, "patchify: batch %d must be at least 1, the patch size %d 1 .. 64 and the image %d x %d at least one patch", B, p, th, tw);
  if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(out) & 15))
    return set_err(VD3D_E_UNSUPPORTED, "patchify: the rows must be 16-byte aligned (the image 4-byte)");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_patchify_f32(c->stream, x, B, th, tw, p, out)) return set_err(VD3D_E_UNSUPPORTED, "patchify: too many rows for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_im2col_nhwc_f32(vd3d_ctx* c, const float* x, int B, int H, int W, int C, int k, int stride, int pt, int pb, int pl, int pr, float* rows) {
  if (!c || !x || !rows) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_im2col_nhwc_f32(c->stream, x, B, H, W, C, k, stride, pt, pb, pl, pr, rows))
    return set_err(VD3D_E_UNSUPPORTED, "im2col: not built: batch %d, map %d x %d x %d, kernel %d (1 | 3 | 7), stride %d (1 | 2), padding %d / %d / %d / %d (0 .. k - 1 each, "
                   "at least one output pixel), or the rows not 16-byte aligned (x 16-byte where C %% 4 == 0, else 4-byte), or too many rows for one grid",
                   B, H, W, C, k, stride, pt, pb, pl, pr);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_maxpool3x3_s2_nhwc_f32(vd3d_ctx* c, const float* x, int B, int H, int W, int C, int pt, int pb, int pl, int pr, float pad, float* out) {
  if (!c || !x || !out) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_maxpool3x3_s2_nhwc_f32(c->stream, x, B, H, W, C, pt, pb, pl, pr, pad, out))
    return set_err(VD3D_E_UNSUPPORTED, "maxpool3x3_s2: not built: batch %d, map %d x %d x %d (C a multiple of 4), padding %d / %d / %d / %d (0 .. 2 each, at least one "
                   "output pixel), or x / out not 16-byte aligned, or a map too large for one grid", B, H, W, C, pt, pb, pl, pr);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int64_t vd3d_groupnorm_nhwc_f32_workspace_bytes(int B, int64_t P, int C, int G) { return (int64_t)vd_groupnorm_workspace_bytes(B, (long long)P, C, G); }
VD3D_EXPORT int vd3d_groupnorm_nhwc_f32(vd3d_ctx* c, const float* x, const float* res, const float* gamma, const float* beta, float eps, int flags, int B, int64_t P,
                                        int C, int G, void* ws, int64_t ws_bytes, float* out) {
  if (!c || !x || !gamma || !beta || !ws || !out || (flags & ~VD3D_GN_RELU)) return set_err(VD3D_E_INVALID, "bad argument");
  const long long need = vd_groupnorm_workspace_bytes(B, (long long)P, C, G);
  if (need < 0)
    return set_err(VD3D_E_UNSUPPORTED, "groupnorm: shape not built: %d channels in %d groups, batch %d, %lld pixels (built: C in {64, 128, 256, 512, 1024} with C / G in "
                   "{2, 4, 8, 16, 32}, batch 1 .. 65535, up to 2^24 pixels)", C, G, B, (long long)P);
  if (ws_bytes < need) return set_err(VD3D_E_INVALID, "groupnorm: the workspace holds %lld bytes, %lld needed", (long long)ws_bytes, need);
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_groupnorm_nhwc_f32(c->stream, x, res, gamma, beta, eps, flags & VD3D_GN_RELU, B, (long long)P, C, G, ws, out))
    return set_err(VD3D_E_UNSUPPORTED, "groupnorm: x, the residual, gamma, beta, the workspace and out must be 16-byte aligned");
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- DepthPro (vd3d_depthpro.hip): every refusal below returns before anything is launched
#define DP_ALIGN16(p) ((reinterpret_cast<uintptr_t>(p) & 15) == 0)
VD3D_EXPORT int vd3d_depthpro_preprocess_u8(vd3d_ctx* c, const uint8_t* frames_bgr, int B, int H, int W, int S, const float* mean_host, const float* std_host, float* out) {
  if (!c || !frames_bgr || !mean_host || !std_host || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (B < 1 || H < 1 || W < 1 || S < 4 || S % 4)
    return set_err(VD3D_E_UNSUPPORTED, "depthpro_preprocess: batch %d, frame %d x %d and side %d: at least one frame and one pixel, the side a multiple of 4", B, H, W, S);
  if (H > (1 << 20) || W > (1 << 20) || S > (1 << 20)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_preprocess: a side past 2^20 (%d x %d -> %d)", H, W, S);
  for (int i = 0; i < 3; ++i)
    if (!(std_host[i] != 0.f)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_preprocess: std[%d] is zero or NaN", i);
  if (!DP_ALIGN16(out)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_preprocess: the output must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_depthpro_preprocess_u8(c->stream, frames_bgr, B, H, W, S, mean_host, std_host, out)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_preprocess: too many pixels for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_depthpro_post_f32(vd3d_ctx* c, const float* pred, const float* fov_or_null, int B, int S, int oH, int oW, float* out) {
  if (!c || !pred || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (B < 1 || S < 1 || oH < 1 || oW < 1 || S > (1 << 20) || oH > (1 << 20) || oW > (1 << 20))
    return set_err(VD3D_E_UNSUPPORTED, "depthpro_post: empty shape or a side past 2^20: batch %d, prediction %d x %d, output %d x %d", B, S, S, oH, oW);
  if ((reinterpret_cast<uintptr_t>(pred) & 3) || (reinterpret_cast<uintptr_t>(out) & 3) || (reinterpret_cast<uintptr_t>(fov_or_null) & 3))
    return set_err(VD3D_E_UNSUPPORTED, "depthpro_post: the prediction, the field of view and the output must be 4-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_depthpro_post_f32(c->stream, pred, fov_or_null, B, S, oH, oW, out)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_post: too many pixels for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}
// ---- DepthPro's patch pyramid and patch merge (vd3d_depthpro_pyramid.hip)
VD3D_EXPORT int64_t vd3d_depthpro_patches_count(int S, int p, int stride_full, int stride_half, int stride_quarter) {
  return (int64_t)vd_depthpro_patches_count(S, p, stride_full, stride_half, stride_quarter);
}
VD3D_EXPORT int vd3d_depthpro_patches_f32(vd3d_ctx* c, const float* pixel_values, int B, int S, int p, int stride_full, int stride_half, int stride_quarter, float* patches) {
  if (!c || !pixel_values || !patches) return set_err(VD3D_E_INVALID, "bad argument");
  if (B < 1 || S > (1 << 20) || vd_depthpro_patches_count(S, p, stride_full, stride_half, stride_quarter) < 1)
    return set_err(VD3D_E_UNSUPPORTED, "depthpro_patches: batch %d, side %d (a multiple of 4, up to 2^20), patch %d, strides %d / %d / %d: every level must hold a patch "
                   "and a level of several patches needs a stride of at least 1", B, S, p, stride_full, stride_half, stride_quarter);
  if ((reinterpret_cast<uintptr_t>(pixel_values) & 3) || (reinterpret_cast<uintptr_t>(patches) & 3))
    return set_err(VD3D_E_UNSUPPORTED, "depthpro_patches: the pixel values and the patches must be 4-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_depthpro_patches_f32(c->stream, pixel_values, B, S, p, stride_full, stride_half, stride_quarter, patches))
    return set_err(VD3D_E_UNSUPPORTED, "depthpro_patches: too many pixels for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_depthpro_merge_f32(vd3d_ctx* c, const float* rows, int n, int B, int T, int C, int g, int padding, int oh, int ow, float* out) {
  if (!c || !rows || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (n < 1 || B < 1 || C < 1 || g < 1 || g > 4096 || padding < 0 || oh < 1 || ow < 1 || oh > (1 << 20) || ow > (1 << 20) || (long long)T < (long long)g * g || n > (1 << 20))
    return set_err(VD3D_E_UNSUPPORTED, "depthpro_merge: %d sequences per frame, batch %d, %d tokens of %d channels on a %d x %d grid, padding %d, output %d x %d: every "
                   "count at least 1, the tokens at least the grid, the grid side up to 4096, an output side up to 2^20", n, B, T, C, g, g, padding, oh, ow);
  int side, pad;
  if ((long long)vd_depthpro_merge_geometry(n, g, padding, &side, &pad) > (1 << 20)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_merge: a merged side past 2^20");
  if ((reinterpret_cast<uintptr_t>(rows) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_merge: the rows and the output must be 4-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_depthpro_merge_f32(c->stream, rows, n, B, T, C, g, padding, oh, ow, out)) return set_err(VD3D_E_UNSUPPORTED, "depthpro_merge: too many elements for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- ZoeDepth (vd3d_zoedepth.hip): every refusal below returns before anything is launched
#define ZOE_ALIGN(p, n) ((reinterpret_cast<uintptr_t>(p) & ((n) - 1)) == 0)
static bool zoe_overlap(const void* a, long long a_bytes, const void* b, long long b_bytes) {   // b may be NULL
  if (!b) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}
VD3D_EXPORT int vd3d_zoedepth_preprocess_u8(vd3d_ctx* c, const uint8_t* frames_bgr, const float* table_dev, int B, int H, int W, int pad_h, int pad_w, int th, int tw,
                                            const float* mean_host, const float* std_host, float* out) {
  if (!c || !frames_bgr || !table_dev || !mean_host || !std_host || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (B < 1 || H < 1 || W < 1 || th < 1 || tw < 1 || H > (1 << 20) || W > (1 << 20) || th > (1 << 20) || tw > (1 << 20))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_preprocess: empty shape or a side past 2^20: batch %d, frame %d x %d, output %d x %d", B, H, W, th, tw);
  if (pad_h < 0 || pad_w < 0 || pad_h >= H || pad_w >= W)
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_preprocess: a reflect pad of %d x %d on a %d x %d frame: the pad must be smaller than its side", pad_h, pad_w, H, W);
  for (int i = 0; i < 3; ++i)
    if (!(std_host[i] != 0.f)) return set_err(VD3D_E_UNSUPPORTED, "zoedepth_preprocess: std[%d] is zero or NaN", i);
  if (!ZOE_ALIGN(table_dev, 4) || !ZOE_ALIGN(out, 4)) return set_err(VD3D_E_UNSUPPORTED, "zoedepth_preprocess: the table and the output must be 4-byte aligned");
  const long long out_bytes = (long long)B * th * tw * 12;
  if (zoe_overlap(out, out_bytes, frames_bgr, (long long)B * H * W * 3) || zoe_overlap(out, out_bytes, table_dev, 1024))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_preprocess: the output overlaps an input");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_zoedepth_preprocess_u8(c->stream, frames_bgr, table_dev, B, H, W, pad_h, pad_w, th, tw, mean_host, std_host, out))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_preprocess: too many pixels for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_zoedepth_post_f32(vd3d_ctx* c, const float* pred, int B, int th, int tw, int H, int W, int pad_h, int pad_w, float* out) {
  if (!c || !pred || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (B < 1 || H < 1 || W < 1 || th < 1 || tw < 1 || H > (1 << 20) || W > (1 << 20) || th > (1 << 20) || tw > (1 << 20) || pad_h < 0 || pad_w < 0 || pad_h > (1 << 20) || pad_w > (1 << 20))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_post: empty shape, a negative pad or a side past 2^20: batch %d, prediction %d x %d, output %d x %d, pad %d x %d", B, th, tw, H, W,
                   pad_h, pad_w);
  if (!ZOE_ALIGN(pred, 4) || !ZOE_ALIGN(out, 4)) return set_err(VD3D_E_UNSUPPORTED, "zoedepth_post: the prediction and the output must be 4-byte aligned");
  if (zoe_overlap(out, (long long)B * H * W * 4, pred, (long long)B * th * tw * 4)) return set_err(VD3D_E_UNSUPPORTED, "zoedepth_post: the output overlaps the prediction");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_zoedepth_post_f32(c->stream, pred, B, th, tw, H, W, pad_h, pad_w, out)) return set_err(VD3D_E_UNSUPPORTED, "zoedepth_post: too many pixels for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_zoedepth_attractor_f32(vd3d_ctx* c, const float* attractors, const float* prev_bins, int B, int h, int w, int hp, int wp, int nA, int nb, int mean,
                                            float* out) {
  if (!c || !attractors || !prev_bins || !out) return set_err(VD3D_E_INVALID, "bad argument");
  if (B < 1 || h < 1 || w < 1 || hp < 1 || wp < 1 || h > (1 << 15) || w > (1 << 15) || hp > (1 << 15) || wp > (1 << 15))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_attractor: empty shape or a side past 2^15: batch %d, map %d x %d, previous map %d x %d", B, h, w, hp, wp);
  if (nA < 1 || nA > 16 || nb < 4 || nb > 256 || nb % 4)
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_attractor: %d attractors and %d bins: built for 1 .. 16 attractors and a multiple of 4 up to 256 bins", nA, nb);
  if (!ZOE_ALIGN(attractors, 4) || !ZOE_ALIGN(prev_bins, 16) || !ZOE_ALIGN(out, 16))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_attractor: the bins (in and out) must be 16-byte aligned, the attractors 4-byte aligned");
  const long long out_bytes = (long long)B * h * w * nb * 4;
  if (zoe_overlap(out, out_bytes, prev_bins, (long long)B * hp * wp * nb * 4) || zoe_overlap(out, out_bytes, attractors, (long long)B * h * w * nA * 4))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_attractor: the output overlaps an input");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_zoedepth_attractor_f32(c->stream, attractors, prev_bins, B, h, w, hp, wp, nA, nb, mean != 0, out))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_attractor: too many elements for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_zoedepth_bins_f32(vd3d_ctx* c, const float* last, const float* rel_or_null, const float* wrel_or_null, const float* P, const float* bins,
                                       const float* w1_last, const float* b1, const float* w2, const float* b2, const float* table, double min_temp, double max_temp, int B,
                                       int H, int W, int hc, int wc, int Ch, int nb, float* out) {
  if (!c || !last || !P || !bins || !w1_last || !b1 || !w2 || !b2 || !table || !out || (rel_or_null == nullptr) != (wrel_or_null == nullptr))
    return set_err(VD3D_E_INVALID, "bad argument");
  if (B < 1 || H < 1 || W < 1 || hc < 1 || wc < 1 || H > (1 << 15) || W > (1 << 15) || hc > (1 << 15) || wc > (1 << 15))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_bins: empty shape or a side past 2^15: batch %d, map %d x %d, coarse map %d x %d", B, H, W, hc, wc);
  if (Ch < 4 || Ch > 128 || Ch % 4 || nb < 4 || nb > 256 || nb % 4)
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_bins: %d hidden channels and %d bins: built for a multiple of 4 up to 128 hidden channels and a multiple of 4 up to 256 bins "
                   "(the feature map has 32 channels)", Ch, nb);
  if (!(min_temp > 0.0) || !(max_temp >= min_temp)) return set_err(VD3D_E_UNSUPPORTED, "zoedepth_bins: temperatures %g .. %g: 0 < min_temp <= max_temp", min_temp, max_temp);
  if (!ZOE_ALIGN(last, 16) || !ZOE_ALIGN(P, 16) || !ZOE_ALIGN(bins, 16))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_bins: the feature map, the projected embedding and the bins must be 16-byte aligned");
  if (!ZOE_ALIGN(rel_or_null, 4) || !ZOE_ALIGN(wrel_or_null, 4) || !ZOE_ALIGN(w1_last, 4) || !ZOE_ALIGN(b1, 4) || !ZOE_ALIGN(w2, 4) || !ZOE_ALIGN(b2, 4) || !ZOE_ALIGN(table, 4) ||
      !ZOE_ALIGN(out, 4))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_bins: the plane, the weights, the table and the output must be 4-byte aligned");
  const long long out_bytes = (long long)B * H * W * 4, coarse = (long long)B * hc * wc * 4;
  if (zoe_overlap(out, out_bytes, last, out_bytes * 32) || zoe_overlap(out, out_bytes, rel_or_null, out_bytes) || zoe_overlap(out, out_bytes, P, coarse * Ch) ||
      zoe_overlap(out, out_bytes, bins, coarse * nb))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_bins: the output overlaps an input");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_zoedepth_bins_f32(c->stream, last, rel_or_null, wrel_or_null, P, bins, w1_last, b1, w2, b2, table, min_temp, max_temp - min_temp, B, H, W, hc,
                                   wc, Ch, nb, out))
    return set_err(VD3D_E_UNSUPPORTED, "zoedepth_bins: too many pixels for one grid");
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_preview_image(vd3d_ctx* c, int type, const uint8_t* left_bgr, const uint8_t* right_bgr, int h, int w, uint8_t* out_bgr) {
  if (!c || !left_bgr || !right_bgr || !out_bgr || h < 1 || w < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (!vd_launch_preview(c->stream, type, left_bgr, right_bgr, h, w, out_bgr))
    return set_err(VD3D_E_UNSUPPORTED, "preview type %d (colour-mapped heat-maps / arrow overlay need OpenCV's tables and rasteriser)", type);
  HIPCHK(hipGetLastError());
  return 0;
}

// the colour-mapped previews of generate_preview_image (core/preview_utils.py:42-66); lut_bgr_dev: the caller's 256 x 3 BGR table in HBM
VD3D_EXPORT int vd3d_preview_heatmap(vd3d_ctx* c, int type, const float* shift_map, int h, int w, const uint8_t* lut_bgr_dev, uint8_t* out_bgr) {
  if (!c || !shift_map || !lut_bgr_dev || !out_bgr || h < 1 || w < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (c->mm_cap < 1) { HIPCHK(re_alloc(&c->mm, (size_t)3)); c->mm_cap = 1; }
  if (!vd_launch_preview_heatmap(c->stream, type, shift_map, h, w, lut_bgr_dev, c->mm, out_bgr))
    return set_err(VD3D_E_UNSUPPORTED, "heat-map type %d (0 shift, 1 |shift|, 2 clipped, 3 feather mask)", type);
  HIPCHK(hipGetLastError());
  return 0;
}

// body layer of the up-scale network on the matrix cores (vd3d_conv.hip)
VD3D_EXPORT int vd3d_conv3x3_c64_f16(vd3d_ctx* c, const void* x_nhwc, int H, int W, const void* w_frag, const float* bias, const float* slope_or_null,
                                     void* y_nhwc) {
  if (!c || !x_nhwc || !w_frag || !bias || !y_nhwc || H < 1 || W < 1 || x_nhwc == y_nhwc) return set_err(VD3D_E_INVALID, "bad argument");
  if ((long long)H * W * 128 >= (1ll << 32)) return set_err(VD3D_E_INVALID, "conv3x3_c64_f16: activation larger than 4 GB");
  if (((uintptr_t)x_nhwc | (uintptr_t)y_nhwc | (uintptr_t)w_frag | (uintptr_t)bias | (uintptr_t)slope_or_null) & 15)
    return set_err(VD3D_E_INVALID, "conv3x3_c64_f16: pointers must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "conv3x3");
  if (!vd_launch_conv3x3_c64_f16(c->stream, x_nhwc, H, W, w_frag, bias, slope_or_null, y_nhwc)) return set_err(VD3D_E_HIP, "conv3x3_c64_f16: LDS attribute");
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_conv3x3_head_f16(vd3d_ctx* c, const void* x_nhwc3, int H, int W, const float* w27x64, const float* bias, const float* slope_or_null,
                                      void* y_nhwc64) {
  if (!c || !x_nhwc3 || !w27x64 || !bias || !y_nhwc64 || H < 1 || W < 1) return set_err(VD3D_E_INVALID, "conv3x3_head_f16: bad argument");
  if ((long long)H * W * 128 >= (1ll << 32)) return set_err(VD3D_E_INVALID, "conv3x3_head_f16: activation larger than 4 GB");
  if ((reinterpret_cast<uintptr_t>(y_nhwc64) | reinterpret_cast<uintptr_t>(w27x64)) & 15) return set_err(VD3D_E_INVALID, "conv3x3_head_f16: y and w must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "conv_head");
  vd_launch_conv3x3_head_f16(c->stream, x_nhwc3, H, W, w27x64, bias, slope_or_null, y_nhwc64);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_esr_tail_f32(vd3d_ctx* c, const void* t_nhwc64, const void* x_nhwc3, int H, int W, int r, float* out_planar) {
  if (!c || !t_nhwc64 || !x_nhwc3 || !out_planar || H < 1 || W < 1 || (r != 2 && r != 4)) return set_err(VD3D_E_INVALID, "esr_tail_f32: bad argument (r = 2 or 4)");
  if (reinterpret_cast<uintptr_t>(t_nhwc64) & 15) return set_err(VD3D_E_INVALID, "esr_tail_f32: t must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "esr_tail");
  vd_launch_esr_tail_f32(c->stream, t_nhwc64, x_nhwc3, H, W, r, out_planar);
  HIPCHK(hipGetLastError());
  return 0;
}

// the RRDBNet convolutions (vd3d_conv_rdb.hip): every rule of include/vd3d.h is checked here, before anything is launched
VD3D_EXPORT int vd3d_conv3x3_dense_f16(vd3d_ctx* c, const void* x, int H, int W, int x_stride, int Cin, const void* w_frag, const float* bias, int Cout,
                                       float slope, float alpha, const void* r1_or_null, int r1_stride, float beta, const void* r2_or_null, int r2_stride,
                                       int up2, void* y, int y_stride, int y_offset) {
  if (!c || !x || !w_frag || !bias || !y) return set_err(VD3D_E_INVALID, "conv3x3_dense_f16: null argument");
  if (H < 1 || W < 1 || H > 32768 || W > 32768) return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: map %d x %d must be 1 .. 32768 on each side", H, W);
  if (Cin != 64 && Cin != 96 && Cin != 128 && Cin != 160 && Cin != 192)
    return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: C_in %d must be one of 64, 96, 128, 160, 192", Cin);
  if (Cout != 32 && Cout != 64) return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: C_out %d must be 32 or 64", Cout);
  if (x_stride < Cin || (x_stride & 7)) return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: x_stride %d must be a multiple of 8 and >= C_in %d", x_stride, Cin);
  if (y_offset < 0 || (y_offset & 7) || (y_stride & 7) || y_stride < y_offset + Cout)
    return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: y_offset %d and y_stride %d must be multiples of 8 with y_offset + C_out %d <= y_stride", y_offset, y_stride, Cout);
  if ((r1_or_null && (r1_stride < Cout || (r1_stride & 7))) || (r2_or_null && (r2_stride < Cout || (r2_stride & 7))))
    return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: a residual's stride must be a multiple of 8 and >= C_out %d", Cout);
  if (up2 && (Cin != 64 || Cout != 64 || (H & 1) || (W & 1)))
    return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: up2 is built for 64 -> 64 channels and an even output size (got %d -> %d, %d x %d)", Cin, Cout, H, W);
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w_frag | (uintptr_t)bias | (uintptr_t)r1_or_null | (uintptr_t)r2_or_null) & 15)
    return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: pointers must be 16-byte aligned");
  const long long in_pix = up2 ? (long long)(H / 2) * (W / 2) : (long long)H * W, out_pix = (long long)H * W;
  {   // the bytes read (channels [0, C_in) of every input pixel) and the bytes written (the output slice of every pixel) must not meet: with one base
      // pointer and one stride that is the channel test of the header; any other overlap of the two extents is refused as well
    const uintptr_t xb = (uintptr_t)x, xe = xb + (uintptr_t)(((in_pix - 1) * x_stride + Cin) * 2);
    const uintptr_t yb = (uintptr_t)y + (uintptr_t)y_offset * 2, ye = (uintptr_t)y + (uintptr_t)(((out_pix - 1) * y_stride + y_offset + Cout) * 2);
    const bool same_grid = x == y && x_stride == y_stride && !up2;
    if (same_grid ? y_offset < Cin : (xb < ye && yb < xe))
      return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: the output slice [%d, %d) meets the input channels [0, %d) of the same buffer (a race between workgroups)",
                     y_offset, y_offset + Cout, Cin);
    const void* rs[2] = {r1_or_null, r2_or_null};
    const int rst[2] = {r1_stride, r2_stride};
    for (int i = 0; i < 2; ++i) {
      if (!rs[i]) continue;
      const uintptr_t rb = (uintptr_t)rs[i], re = rb + (uintptr_t)(((out_pix - 1) * rst[i] + Cout) * 2);
      const bool rgrid = rs[i] == y && rst[i] == y_stride;
      if (rgrid ? y_offset < Cout : (rb < ye && yb < re))
        return set_err(VD3D_E_UNSUPPORTED, "conv3x3_dense_f16: residual %d overlaps the output slice", i + 1);
    }
  }
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "conv3x3_dense");
  if (!vd_launch_conv3x3_dense_f16(c->stream, x, H, W, x_stride, Cin, w_frag, bias, Cout, slope, alpha, r1_or_null, r1_stride, beta, r2_or_null, r2_stride,
                                   up2 ? 1 : 0, y, y_stride, y_offset))
    return set_err(VD3D_E_HIP, "conv3x3_dense_f16: the dynamic LDS opt-in failed");
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_nhwc_f16_to_planar3_f32(vd3d_ctx* c, const void* t_nhwc32, int H, int W, float* out_planar) {
  if (!c || !t_nhwc32 || !out_planar) return set_err(VD3D_E_INVALID, "nhwc_f16_to_planar3_f32: null argument");
  if (H < 1 || W < 1 || H > 32768 || W > 32768) return set_err(VD3D_E_UNSUPPORTED, "nhwc_f16_to_planar3_f32: map %d x %d must be 1 .. 32768 on each side", H, W);
  if (((uintptr_t)t_nhwc32 & 15) || ((uintptr_t)out_planar & 3)) return set_err(VD3D_E_UNSUPPORTED, "nhwc_f16_to_planar3_f32: t must be 16-byte and out 4-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "esr_tail");
  vd_launch_nhwc_f16_to_planar3_f32(c->stream, t_nhwc32, H, W, out_planar);
  HIPCHK(hipGetLastError());
  return 0;
}

// optional NV12 wire format at the frame I/O boundary (vd3d_nv12.hip)
VD3D_EXPORT int vd3d_nv12_to_bgr(vd3d_ctx* c, const uint8_t* y_plane, long long y_pitch, const uint8_t* uv_plane, long long uv_pitch, int h, int w,
                                 uint8_t* out_bgr) {
  if (!c || !y_plane || !uv_plane || !out_bgr || h < 2 || w < 2 || (h & 1) || (w & 1) || y_pitch < w || uv_pitch < w)
    return set_err(VD3D_E_INVALID, "bad argument (NV12 needs even h and w)");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "nv12_in");
  vd_launch_nv12_to_bgr(c->stream, y_plane, uv_plane, h, w, y_pitch, uv_pitch, out_bgr);
  HIPCHK(hipGetLastError());
  return 0;
}
VD3D_EXPORT int vd3d_bgr_to_nv12(vd3d_ctx* c, const uint8_t* bgr, int h, int w, uint8_t* y_plane, long long y_pitch, uint8_t* uv_plane,
                                 long long uv_pitch) {
  if (!c || !y_plane || !uv_plane || !bgr || h < 2 || w < 2 || (h & 1) || (w & 1) || y_pitch < w || uv_pitch < w)
    return set_err(VD3D_E_INVALID, "bad argument (NV12 needs even h and w)");
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "nv12_out");
  vd_launch_bgr_to_nv12(c->stream, bgr, h, w, y_plane, uv_plane, y_pitch, uv_pitch);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_preview_arrows(vd3d_ctx* c, const uint8_t* left_bgr, const float* shift_map, int h, int w, uint8_t* out_bgr) {
  if (!c || !left_bgr || !shift_map || !out_bgr || h < 1 || w < 1 || left_bgr == out_bgr) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  vd_launch_preview_arrows(c->stream, left_bgr, shift_map, h, w, out_bgr);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_detect_black_bars(vd3d_ctx* c, const uint8_t* frame_bgr, int h, int w, int* top_host, int* bottom_host) {
  if (!c || !frame_bgr || !top_host || !bottom_host || h < 1 || w < 1) return set_err(VD3D_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (h > c->rowflag_cap) { HIPCHK(re_alloc(&c->rowflag, (size_t)h)); c->rowflag_cap = h; }
  vd_launch_autocrop(c->stream, frame_bgr, h, w, 16.0 / 9.0, c->rowflag, c->work);
  c->crop_scalars_dirty = true;
  int32_t tb[2];
  HIPCHK(hipMemcpyAsync(tb, &c->work->fs.crop_top, sizeof tb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *top_host = tb[0]; *bottom_host = tb[1];
  return 0;
}

VD3D_EXPORT int vd3d_stream_copy(vd3d_ctx* c, const void* src, void* dst, size_t bytes) {
  HIPCHK(hipSetDevice(c->device));
  StageTimer t(c, "stream_copy");
  vd_launch_stream_copy(c->stream, src, dst, bytes);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_torch_math(vd3d_ctx* c, int op, const float* x, float param, float* out, long long n) {
  if (!c) return set_err(VD3D_E_INVALID, "NULL context");
  if (op < 0 || op > 2 || n < 0 || (n > 0 && (!x || !out))) return set_err(VD3D_E_INVALID, "vd3d_torch_math: op 0..2, n >= 0, device pointers");
  HIPCHK(hipSetDevice(c->device));
  if (n) vd_launch_torch_math(c->stream, op, x, param, out, n);
  HIPCHK(hipGetLastError());
  return 0;
}

VD3D_EXPORT int vd3d_torch_math_aten(vd3d_ctx* c, int op, const float* x, double param, float* out, long long n, int aten_threads) {
  if (!c) return set_err(VD3D_E_INVALID, "NULL context");
  if (op < 0 || op > 1 || n < 0 || n >= (1ll << 32) || (n > 0 && (!x || !out)))
    return set_err(VD3D_E_INVALID, "vd3d_torch_math_aten: op 0..1, 0 <= n < 2^32, device pointers");
  HIPCHK(hipSetDevice(c->device));
  if (n) vd_launch_torch_math_aten(c->stream, op, x, param, out, n, aten_threads);
  HIPCHK(hipGetLastError());
  return 0;
}

// development probe (tools/probe_step.py): 0 = workgroup divisor of the batched chain kernels, 1 = frames per P3 group
// Process-wide launch-policy switches.  The PRODUCT library keeps the two ROUTE selectors the parity tests use to prove that two code paths give the same
// bytes (3: fused / unfused finishing routes, 4: the long way round feather_strength 0) -- plain ints written before any frame is in flight, read per call;
// everything else (tile heights, tile orders, the parked persistent kernels, chain grouping) exists only in development libraries built with
// -DVD3D_DEV_KNOBS (tools/build_ab.sh dev -DVD3D_DEV_KNOBS), and so does the VD3D_TUNE environment variable (round 6).
// which == -1: query -- 0 when the development knobs are compiled in, VD3D_E_UNSUPPORTED when not.
VD3D_EXPORT int vd3d_debug_tune(int which, int value) {
  if (which == 3) { g_fused_fit = value; return 0; }
  if (which == 4) { g_feather0_long = value; return 0; }
#ifdef VD3D_DEV_KNOBS
  if (which == -1) return 0;
  if (which == 0) vd_set_batch_grid_div(value);
  else if (which == 1) g_chain_group = value;
  else if (which == 2) vd_set_warp_pre_th(value);
  else if (which == 5) vd_set_conv_mode(value);
  else if (which == 6) vd_set_finish_persist(value);
  else if (which == 7) vd_set_warp_nofeather_th(value);
  else if (which == 8) vd_set_finish_xcd(value);
  else if (which == 9) vd_set_warp_order(value);
  else return set_err(VD3D_E_INVALID, "vd3d_debug_tune: unknown knob %d", which);
  return 0;
#else
  (void)value;
  if (which == -1 || (which >= 0 && which <= 9)) return set_err(VD3D_E_UNSUPPORTED, "vd3d_debug_tune(%d): development knob, this library was built without -DVD3D_DEV_KNOBS", which);
  return set_err(VD3D_E_INVALID, "vd3d_debug_tune: unknown knob %d", which);
#endif
}

VD3D_EXPORT int vd3d_set_profiling(vd3d_ctx* c, int enable) {
  vd3d_sync(c);
  c->profiling = enable != 0;
  if (enable) c->acc.clear();
  return 0;
}
// average milliseconds per call of the named stage since profiling was enabled; -1 if never seen.  Synchronises.
VD3D_EXPORT float vd3d_last_stage_ms(vd3d_ctx* c, const char* stage) {
  vd3d_sync(c);
  auto it = c->acc.find(stage);
  if (it == c->acc.end() || it->second.second == 0) return -1.f;
  return (float)(it->second.first / (double)it->second.second);
}
VD3D_EXPORT long vd3d_stage_calls(vd3d_ctx* c, const char* stage) {
  vd3d_sync(c);
  auto it = c->acc.find(stage);
  return it == c->acc.end() ? 0 : it->second.second;
}
