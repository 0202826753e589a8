// vd3d_conv_head.hip -- the DPT head's 3 x 3 convolutions with their up-sampling in front (and, for conv2, everything behind) in ONE exact-float32 kernel:
//
//     y = conv3x3( up(x) + b_in )            up = bilinear, align_corners=True, [ih, iw] -> [oh, ow]; zero padding 1, stride 1, no bias of its own
//     TAIL:  out[p] = max(b3 + sum_c w3[c] * max(y[p][c] + b2[c], 0), 0) * scale        (vd3d_dpt_head_tail_f32's function, one float per pixel)
//     plain: out = y, NHWC
//
// It replaces three launches (k_upsample_bilinear_bias_nhwc_f32, the library convolution, k_head_tail) whose two intermediate maps -- [oh][ow][C_IN] and
// [oh][ow][C_OUT] -- existed only to be read once.  Arithmetic: float32 operands on v_mfma_f32_32x32x2_f32, float32 accumulation: k_attn_f32's class, not a
// split-operand mode.  No split-K, no atomics: every output is summed by one lane in one fixed K order, identical from run to run.
//
// Implicit GEMM per workgroup: an 8 x 32 output tile (k_conv_x3's geometry, vd3d_conv_x3.hip), 512 threads = 8 waves, wave w = tile row w.  Output channels are the MFMA's M
// side (A[i = lane & 31 = channel][k = lane >> 5]), the row's 32 pixels its N side (B[k = lane >> 5][j = lane & 31 = pixel]): a lane's 16 accumulator
// registers are channels (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of ONE pixel, so the tail's dot product is an in-lane sum plus one exchange with lane ^ 32.
// K order (fixed): 16-channel chunk (outer), tap 0 .. 8 (dy major), channel group g = 0, 1 of the chunk, j = 0 .. 3; one MFMA sums channels 8 g + j (k = 0)
// and 8 g + 4 + j (k = 1) of the chunk.  Blocked: within a chunk the steps with j even and with j odd are two fmaf chains from zero, and
// total = (total + even) + odd behind the chunk.
//   interpolated operand: per chunk the tile + 1 halo ring (10 x 34 pixels x 16 channels) is computed ONCE from the low-resolution map -- four 16-byte global
//     loads per (pixel, 4-channel quad), issued a chunk ahead and held in registers under the MFMAs -- with k_upsample_bilinear_bias_nhwc_f32's exact operation
//     order ((ly0 (lx0 p00 + lx1 p01) + ly1 (lx0 p10 + lx1 p11)) + b, no contraction: the Makefile's -ffp-contract=off), positions outside the up-sampled map
//     exactly 0 (the convolution's padding, not bias), into LDS [quad 4][pixel slot 388][4 floats] (24 832 B, double-buffered).  All nine taps read their B
//     fragments from it: 32 consecutive pixels shifted by the tap = consecutive 16-byte slots, one ds_read_b128 per four MFMAs.
//   weights: packed once per module into [chunk][tap][quad 4][oc C_OUT][4 floats]; a chunk's 9 x 4 x C_OUT x 16 bytes (18 432 / 36 864) go through registers
//     into a double-buffered LDS image, A fragments by ds_read_b128.
//   The next chunk's interpolation and LDS stores are spread between the taps of the current one (VALU work in the shadow of the 64-cycle MFMAs); one
//     barrier per chunk: buffer (c + 1) & 1 was last read in chunk c - 1, in front of that chunk's barrier.
//   LDS (dynamic only): 2 x 24 832 + 2 x 24 576 = 98 816 (C_OUT 32), 2 x 24 832 + 2 x 40 960 = 131 584 (C_OUT 64; the weight buffers padded to whole 512-thread rounds): one workgroup, two waves per SIMD.
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include "vd3d_x3.h"

typedef float ch_f4 __attribute__((ext_vector_type(4)));   // native vectors: the register images of the loads below stay SSA values (HIP's float4 arrays went to scratch)

#define CH_TH 8
#define CH_TW 32
#define CH_PW (CH_TW + 2)
#define CH_NPIX ((CH_TH + 2) * CH_PW)                     // 340
#define CH_NT 512
#define CH_PLANE 388                                      // pixel slots of a quad plane: >= 3 x 512 / 4 (every item of a thread has a slot: stores without a branch), 16 banks apart
#define CH_X_BUF (4 * CH_PLANE * 16)                      // one interpolated chunk: 24 832 bytes
#define CH_ITEMS (CH_NPIX * 4)                            // (pixel, quad) items of a chunk: 1 360
#define CH_ITERS ((CH_ITEMS + CH_NT - 1) / CH_NT)         // 3 per thread
__host__ __device__ constexpr int ch_w_buf(int cout) { return 9 * 4 * cout * 16; }
__host__ __device__ constexpr int ch_w_lds(int cout) { return (ch_w_buf(cout) + CH_NT * 16 - 1) / (CH_NT * 16) * (CH_NT * 16); }   // whole 512-thread rounds: 24 576 / 40 960
__host__ __device__ constexpr int ch_lds(int cout) { return 2 * CH_X_BUF + 2 * ch_w_lds(cout); }
static_assert(ch_lds(32) == 98816 && ch_lds(64) == 131584 && ch_lds(64) <= 163840 && CH_PLANE * 4 >= CH_ITERS * CH_NT && CH_ITERS == 3, "LDS plan");

struct vd_ch_args {
  int ih, iw, oh, ow;
  float sh, sw;       // (ih - 1) / (oh - 1), (iw - 1) / (ow - 1): vd_launch_upsample_bilinear_bias_nhwc_f32's
  int ntx;            // tiles per output row
  float b3, scale;    // TAIL
};

template <int C_IN, int C_OUT, bool TAIL>
__global__ __launch_bounds__(CH_NT) void k_conv3x3_up_f32(const float* __restrict__ X, const float* __restrict__ bin, const float* __restrict__ Wimg,
                                                          const float* __restrict__ b2, const float* __restrict__ w3, float* __restrict__ out, vd_ch_args a) {
  constexpr int NM = C_OUT / 32, NCHUNK = C_IN / 16, WBUF = ch_w_buf(C_OUT), WLDS = ch_w_lds(C_OUT), W_ITEMS = WBUF / 16, W_ITERS = (W_ITEMS + CH_NT - 1) / CH_NT;
  extern __shared__ __attribute__((aligned(16))) uint8_t ch_smem[];   // the only LDS object: [X buffer 0][X buffer 1][W buffer 0][W buffer 1]
  const int tile = blockIdx.x, b = blockIdx.y;
  const int tyi = tile / a.ntx, txi = tile - tyi * a.ntx;
  const int y0 = tyi * CH_TH, x0 = txi * CH_TW;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kh = lane >> 5;
  const float* xb = X + (size_t)b * a.ih * a.iw * C_IN;

  // ---- the interpolation items of this thread: i = it * 512 + tid -> (pixel = i >> 2 of the 10 x 34 halo tile, quad = i & 3 = tid & 3); chunk-invariant
  // corner offsets (floats, from the frame's base) and weights.  A position outside the up-sampled map is the convolution's zero padding.
  int o00[CH_ITERS], o01[CH_ITERS], o10[CH_ITERS], o11[CH_ITERS], dst[CH_ITERS];
  float ly1[CH_ITERS], lx1[CH_ITERS];
  bool inside[CH_ITERS];
#pragma unroll
  for (int it = 0; it < CH_ITERS; ++it) {
    const int i = it * CH_NT + tid, pix = i >> 2, q = i & 3;
    const int py = pix / CH_PW, px = pix - py * CH_PW;
    const int gy = y0 - 1 + py, gx = x0 - 1 + px;
    inside[it] = i < CH_ITEMS && gy >= 0 && gy < a.oh && gx >= 0 && gx < a.ow;
    const int cy = inside[it] ? gy : 0, cx = inside[it] ? gx : 0;
    const float fy = a.sh * (float)cy, fx = a.sw * (float)cx;
    const int yy0 = (int)fy, xx0 = (int)fx;
    const int yy1 = yy0 + (yy0 < a.ih - 1 ? 1 : 0), xx1 = xx0 + (xx0 < a.iw - 1 ? 1 : 0);
    ly1[it] = fy - (float)yy0; lx1[it] = fx - (float)xx0;
    o00[it] = (yy0 * a.iw + xx0) * C_IN + q * 4; o01[it] = (yy0 * a.iw + xx1) * C_IN + q * 4;
    o10[it] = (yy1 * a.iw + xx0) * C_IN + q * 4; o11[it] = (yy1 * a.iw + xx1) * C_IN + q * 4;
    dst[it] = (q * CH_PLANE + pix) * 16;   // items past the halo tile land in the unused slots 340 .. 383 of their plane
  }
  ch_f4 p00[CH_ITERS], p01[CH_ITERS], p10[CH_ITERS], p11[CH_ITERS], wv[W_ITERS], bq;
  auto load = [&](int chunk) {
#pragma unroll
    for (int it = 0; it < CH_ITERS; ++it) {
      p00[it] = *reinterpret_cast<const ch_f4*>(xb + o00[it] + chunk * 16); p01[it] = *reinterpret_cast<const ch_f4*>(xb + o01[it] + chunk * 16);
      p10[it] = *reinterpret_cast<const ch_f4*>(xb + o10[it] + chunk * 16); p11[it] = *reinterpret_cast<const ch_f4*>(xb + o11[it] + chunk * 16);
    }
    bq = *reinterpret_cast<const ch_f4*>(bin + chunk * 16 + (tid & 3) * 4);
#pragma unroll
    for (int p = 0; p < W_ITERS; ++p)   // unconditional (the items past the image re-read its last one): the values stay in registers
      wv[p] = *reinterpret_cast<const ch_f4*>(Wimg + (size_t)chunk * (WBUF / 4) + (p * CH_NT + tid < W_ITEMS ? p * CH_NT + tid : W_ITEMS - 1) * 4);
  };
  auto interp = [&](int it, int buf) {   // k_upsample_bilinear_bias_nhwc_f32's operation order, bit for bit
    // the loaded values pass through an empty volatile asm: their arithmetic stays behind the fence in front of this call (pure ALU work is not ordered by it)
    asm volatile("" : "+v"(p00[it]), "+v"(p01[it]), "+v"(p10[it]), "+v"(p11[it]));
    const float l_y1 = ly1[it], l_y0 = 1.f - l_y1, l_x1 = lx1[it], l_x0 = 1.f - l_x1;
    ch_f4 o;
    o.x = (l_y0 * (l_x0 * p00[it].x + l_x1 * p01[it].x) + l_y1 * (l_x0 * p10[it].x + l_x1 * p11[it].x)) + bq.x;
    o.y = (l_y0 * (l_x0 * p00[it].y + l_x1 * p01[it].y) + l_y1 * (l_x0 * p10[it].y + l_x1 * p11[it].y)) + bq.y;
    o.z = (l_y0 * (l_x0 * p00[it].z + l_x1 * p01[it].z) + l_y1 * (l_x0 * p10[it].z + l_x1 * p11[it].z)) + bq.z;
    o.w = (l_y0 * (l_x0 * p00[it].w + l_x1 * p01[it].w) + l_y1 * (l_x0 * p10[it].w + l_x1 * p11[it].w)) + bq.w;
    if (!inside[it]) o = ch_f4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<ch_f4*>(ch_smem + buf * CH_X_BUF + dst[it]) = o;
  };
  auto put_w = [&](int buf) {   // every thread stores every round (the items past the image fill the buffer's padding): no branch between the MFMAs
#pragma unroll
    for (int p = 0; p < W_ITERS; ++p) *reinterpret_cast<ch_f4*>(ch_smem + 2 * CH_X_BUF + buf * WLDS + (p * CH_NT + tid) * 16) = wv[p];
  };

  x3_f16 tot[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[m][r] = 0.f;

  load(0);
#pragma unroll
  for (int it = 0; it < CH_ITERS; ++it) interp(it, 0);
  put_w(0);
  __syncthreads();

  // fragment bases: B: quad plane kh (+ 2 g), tile row wave (+ 1 halo + dy), column li (+ 1 + dx); A: tap, quad plane kh (+ 2 g), output channel li (+ 32 m)
  const int fx_base = (kh * CH_PLANE + (wave + 1) * CH_PW + li + 1) * 16;
  const int fw_base = 2 * CH_X_BUF + (kh * C_OUT + li) * 16;
#pragma unroll 1
  for (int chunk = 0; chunk < NCHUNK; ++chunk) {
    const int cur = chunk & 1, nxt = cur ^ 1;
    load(chunk + 1 < NCHUNK ? chunk + 1 : chunk);   // straight-line code: behind the last chunk a harmless rebuild of the buffer nobody reads again
    __builtin_amdgcn_sched_barrier(0);              // the loads are issued HERE, a chunk of MFMAs in front of their use (the scheduler sinks them to it otherwise)
    const uint8_t* xs = ch_smem + cur * CH_X_BUF + fx_base;
    const uint8_t* ws = ch_smem + cur * WLDS + fw_base;
    // Blocked summation: a chunk's 72 K = 2 steps go into two fresh accumulators (j even / j odd), added to the running total behind the chunk.  One chain
    // over all of K measured 1.6 x the library path's RMS error against float64 (the rounding of a float32 fmaf chain grows with its length and with the
    // magnitude of its partial sums); chains of 36 steps whose sums meet in C_IN / 8 additions stay below it (tests/test_hip_dpt_head_f32.py).
    x3_f16 acc[2][NM];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][m][r] = acc[1][m][r] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const ch_f4 bf = *reinterpret_cast<const ch_f4*>(xs + (2 * g * CH_PLANE + dy * CH_PW + dx) * 16);
        ch_f4 af[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) af[m] = *reinterpret_cast<const ch_f4*>(ws + ((tap * 4 + 2 * g) * C_OUT + m * 32) * 16);
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[0][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].x, bf.x, acc[0][m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[1][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].y, bf.y, acc[1][m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[0][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].z, bf.z, acc[0][m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[1][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].w, bf.w, acc[1][m], 0, 0, 0);
      }
      // the next chunk's operand images, in the shadow of this chunk's MFMAs
      // (a scheduling fence in front of each piece: the scheduler would otherwise hoist it to the loads, and wait for them there)
      if (tap == 2 || tap == 4 || tap == 6 || tap == 7) __builtin_amdgcn_sched_barrier(0);
      if (tap == 2) interp(0, nxt);
      if (tap == 4) interp(1, nxt);
      if (tap == 6) interp(2, nxt);
      if (tap == 7) put_w(nxt);
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) tot[m] = (tot[m] + acc[0][m]) + acc[1][m];
    __syncthreads();
  }

  // ---- epilogue: accumulator register r of tile m = output channel 32 m + (r & 3) + 8 (r >> 2) + 4 kh of pixel (y0 + wave, x0 + li)
  const int y = y0 + wave, x = x0 + li;
  const bool live = y < a.oh && x < a.ow;
  const size_t pix = ((size_t)b * a.oh + (live ? y : 0)) * a.ow + (live ? x : 0);
  if constexpr (TAIL) {
    float s = 0.f;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const ch_f4 bb = *reinterpret_cast<const ch_f4*>(b2 + 8 * g4 + 4 * kh), ww = *reinterpret_cast<const ch_f4*>(w3 + 8 * g4 + 4 * kh);
      s = vd_fma(fmaxf(tot[0][4 * g4] + bb.x, 0.f), ww.x, s);
      s = vd_fma(fmaxf(tot[0][4 * g4 + 1] + bb.y, 0.f), ww.y, s);
      s = vd_fma(fmaxf(tot[0][4 * g4 + 2] + bb.z, 0.f), ww.z, s);
      s = vd_fma(fmaxf(tot[0][4 * g4 + 3] + bb.w, 0.f), ww.w, s);
    }
    s += __shfl_xor(s, 32, 64);
    if (live && kh == 0) out[pix] = fmaxf(s + a.b3, 0.f) * a.scale;
  } else {
    if (live) {
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
          *reinterpret_cast<ch_f4*>(out + pix * C_OUT + m * 32 + 8 * g4 + 4 * kh) =
              ch_f4{tot[m][4 * g4], tot[m][4 * g4 + 1], tot[m][4 * g4 + 2], tot[m][4 * g4 + 3]};
    }
  }
}

// ---- weights: float32 [Cout][Cin][3][3] -> [chunk][tap][quad 4][oc Cout][4 floats]; one thread = one (chunk, tap, quad, oc): 4 channels
__global__ __launch_bounds__(256) void k_conv3x3_up_pack(const float* __restrict__ W, int Cout, int Cin, float4* __restrict__ img) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int total = (Cin / 16) * 9 * 4 * Cout;
  if (t >= total) return;
  const int oc = t % Cout, q = (t / Cout) & 3, tap = (t / (4 * Cout)) % 9, chunk = t / (36 * Cout);
  const float* w = W + ((size_t)oc * Cin + chunk * 16 + q * 4) * 9 + tap;
  img[t] = make_float4(w[0], w[9], w[18], w[27]);
}

static bool ch_shape_ok(int Cin, int Cout, bool tail) {
  if (tail) return Cout == 32 && (Cin == 32 || Cin == 64 || Cin == 128);
  return Cout == 64 && Cin == 128;
}
long long vd_dpt_head_conv_weight_bytes(int Cin, int Cout) {
  if (!ch_shape_ok(Cin, Cout, true) && !ch_shape_ok(Cin, Cout, false)) return -1;
  return (long long)Cin * 9 * Cout * 4;
}
bool vd_launch_dpt_head_conv_pack(hipStream_t s, const float* W, int Cin, int Cout, void* img) {
  if (vd_dpt_head_conv_weight_bytes(Cin, Cout) < 0 || (reinterpret_cast<uintptr_t>(img) & 15)) return false;
  const int total = (Cin / 16) * 9 * 4 * Cout;
  hipLaunchKernelGGL(k_conv3x3_up_pack, dim3((total + 255) / 256), dim3(256), 0, s, W, Cout, Cin, reinterpret_cast<float4*>(img));
  return true;
}

bool vd_dpt_head_conv_shape_ok(int B, int ih, int iw, int oh, int ow, int Cin, int Cout, bool tail) {
  if (!ch_shape_ok(Cin, Cout, tail) || B < 1 || B > 65535 || ih < 1 || iw < 1 || oh < 2 || ow < 2) return false;
  if ((long long)ih * iw * Cin >= (1ll << 31)) return false;                                   // 32-bit corner offsets inside a frame
  if (((long long)(oh + CH_TH - 1) / CH_TH) * ((ow + CH_TW - 1) / CH_TW) >= (1ll << 31)) return false;
  return true;
}

bool vd_launch_dpt_head_conv_f32(hipStream_t s, const float* x, const float* b_in, int B, int ih, int iw, int oh, int ow, int Cin, const void* wimg, int Cout,
                                 const float* b2, const float* w3, float b3, float scale, float* out) {
  const bool tail = b2 != nullptr;
  if (!vd_dpt_head_conv_shape_ok(B, ih, iw, oh, ow, Cin, Cout, tail)) return false;
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_conv3x3_up_f32<32, 32, true>), ch_lds(32)}, {reinterpret_cast<const void*>(k_conv3x3_up_f32<64, 32, true>), ch_lds(32)},
                     {reinterpret_cast<const void*>(k_conv3x3_up_f32<128, 32, true>), ch_lds(32)}, {reinterpret_cast<const void*>(k_conv3x3_up_f32<128, 64, false>), ch_lds(64)}},
                    attr_set)) return false;
  vd_ch_args a;
  a.ih = ih; a.iw = iw; a.oh = oh; a.ow = ow;
  a.sh = (float)(ih - 1) / (float)(oh - 1); a.sw = (float)(iw - 1) / (float)(ow - 1);
  a.ntx = (ow + CH_TW - 1) / CH_TW;
  a.b3 = b3; a.scale = scale;
  const dim3 grid((unsigned)(a.ntx * ((oh + CH_TH - 1) / CH_TH)), (unsigned)B, 1);
  const float* wi = reinterpret_cast<const float*>(wimg);
  if (!tail) hipLaunchKernelGGL((k_conv3x3_up_f32<128, 64, false>), grid, dim3(CH_NT), ch_lds(64), s, x, b_in, wi, b2, w3, out, a);
  else if (Cin == 32) hipLaunchKernelGGL((k_conv3x3_up_f32<32, 32, true>), grid, dim3(CH_NT), ch_lds(32), s, x, b_in, wi, b2, w3, out, a);
  else if (Cin == 64) hipLaunchKernelGGL((k_conv3x3_up_f32<64, 32, true>), grid, dim3(CH_NT), ch_lds(32), s, x, b_in, wi, b2, w3, out, a);
  else hipLaunchKernelGGL((k_conv3x3_up_f32<128, 32, true>), grid, dim3(CH_NT), ch_lds(32), s, x, b_in, wi, b2, w3, out, a);
  return true;
}
