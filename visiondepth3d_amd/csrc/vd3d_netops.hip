// vd3d_netops.hip -- memory-bound glue kernels of the depth network's transformer blocks (boundary B3; the GEMMs,
// attention and convolutions stay in hipBLASLt / AOTriton / MIOpen as north_star prescribes).
//
// k_add_layernorm:  s = x + y (bf16, rounded like ATen's add), out_norm = LayerNorm(s) * gamma + beta (float32 statistics,
// biased variance, eps inside the sqrt), one wave per row, two rows of traffic instead of ATen's add kernel + layer-norm
// kernel (5 rows).  y == nullptr -> plain LayerNorm.  cols must be a multiple of 128 (2 bf16 per lane per step).
#include "vd3d_dev.h"
#include "vd3d_kernels.h"

VD_DEV float bf2f(uint32_t h) { return __uint_as_float(h << 16); }
VD_DEV uint32_t f2bf(float f) { const uint32_t b = __float_as_uint(f); return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16; }
VD_DEV float wave_sum_f(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int NJ>   // cols = NJ * 128
__global__ __launch_bounds__(256) void k_add_layernorm(const uint32_t* __restrict__ x, const uint32_t* __restrict__ y,
                                                       const uint32_t* __restrict__ gamma, const uint32_t* __restrict__ beta,
                                                       float eps, long long rows, uint32_t* __restrict__ out_sum,
                                                       uint32_t* __restrict__ out_norm) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const size_t base = (size_t)row * (NJ * 64);   // in dwords (2 bf16 each)
  float v[2 * NJ];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const uint32_t a = x[base + lane + 64 * j];
    float lo = bf2f(a & 0xffffu), hi = bf2f(a >> 16);
    if (y) {
      const uint32_t b = y[base + lane + 64 * j];
      const uint32_t slo = f2bf(lo + bf2f(b & 0xffffu)), shi = f2bf(hi + bf2f(b >> 16));
      out_sum[base + lane + 64 * j] = slo | (shi << 16);
      lo = bf2f(slo); hi = bf2f(shi);
    }
    v[2 * j] = lo; v[2 * j + 1] = hi;
    sum += lo + hi;
  }
  const float n = (float)(NJ * 128);
  const float mean = wave_sum_f(sum) / n;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 2 * NJ; ++j) { const float d = v[j] - mean; sq += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum_f(sq) / n + eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const uint32_t g = gamma[lane + 64 * j], b = beta[lane + 64 * j];
    const float lo = (v[2 * j] - mean) * rstd * bf2f(g & 0xffffu) + bf2f(b & 0xffffu);
    const float hi = (v[2 * j + 1] - mean) * rstd * bf2f(g >> 16) + bf2f(b >> 16);
    out_norm[base + lane + 64 * j] = f2bf(lo) | (f2bf(hi) << 16);
  }
}

// float32 variant (the reference runs its HF depth models in float32, core/render_depth.py:758-759): x + y is ATen's exact float32 add,
// LayerNorm statistics two-pass in float32.  One wave per row, float2 per lane per step (cols = NJ * 128).
template <int NJ>
__global__ __launch_bounds__(256) void k_add_layernorm_f32(const float2* __restrict__ x, const float2* __restrict__ y,
                                                           const float2* __restrict__ gamma, const float2* __restrict__ beta,
                                                           float eps, long long rows, float2* __restrict__ out_sum,
                                                           float2* __restrict__ out_norm) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const size_t base = (size_t)row * (NJ * 64);   // in float2
  float v[2 * NJ];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    float2 a = x[base + lane + 64 * j];
    if (y) {
      const float2 b = y[base + lane + 64 * j];
      a.x += b.x; a.y += b.y;
      out_sum[base + lane + 64 * j] = a;
    }
    v[2 * j] = a.x; v[2 * j + 1] = a.y;
    sum += a.x + a.y;
  }
  const float n = (float)(NJ * 128);
  const float mean = wave_sum_f(sum) / n;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 2 * NJ; ++j) { const float d = v[j] - mean; sq += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum_f(sq) / n + eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float2 g = gamma[lane + 64 * j], b = beta[lane + 64 * j];
    out_norm[base + lane + 64 * j] = make_float2((v[2 * j] - mean) * rstd * g.x + b.x, (v[2 * j + 1] - mean) * rstd * g.y + b.y);
  }
}

bool vd_launch_add_layernorm(hipStream_t s, int dtype, const void* x, const void* y, const void* gamma, const void* beta, float eps,
                             long long rows, int cols, void* out_sum, void* out_norm) {
  const dim3 g((unsigned)((rows + 3) / 4)), b(256);
  if (dtype == VD3D_DT_F32) {
    const float2 *xx = (const float2*)x, *yy = (const float2*)y, *gg = (const float2*)gamma, *bb = (const float2*)beta;
    float2 *os = (float2*)out_sum, *on = (float2*)out_norm;
    switch (cols) {
      case 384: hipLaunchKernelGGL(k_add_layernorm_f32<3>, g, b, 0, s, xx, yy, gg, bb, eps, rows, os, on); return true;
      case 768: hipLaunchKernelGGL(k_add_layernorm_f32<6>, g, b, 0, s, xx, yy, gg, bb, eps, rows, os, on); return true;
      case 1024: hipLaunchKernelGGL(k_add_layernorm_f32<8>, g, b, 0, s, xx, yy, gg, bb, eps, rows, os, on); return true;
      default: return false;
    }
  }
  if (dtype != VD3D_DT_BF16) return false;
  const uint32_t *xx = (const uint32_t*)x, *yy = (const uint32_t*)y, *gg = (const uint32_t*)gamma, *bb = (const uint32_t*)beta;
  uint32_t *os = (uint32_t*)out_sum, *on = (uint32_t*)out_norm;
  switch (cols) {
    case 384: hipLaunchKernelGGL(k_add_layernorm<3>, g, b, 0, s, xx, yy, gg, bb, eps, rows, os, on); return true;
    case 768: hipLaunchKernelGGL(k_add_layernorm<6>, g, b, 0, s, xx, yy, gg, bb, eps, rows, os, on); return true;
    case 1024: hipLaunchKernelGGL(k_add_layernorm<8>, g, b, 0, s, xx, yy, gg, bb, eps, rows, os, on); return true;
    default: return false;
  }
}

// k_upsample_bilinear_nhwc: F.interpolate(mode="bilinear", align_corners=True) on a bf16 channels_last tensor (the five
// up-samplings of the DPT neck / head).  One thread = 8 channels (16 B) of one output pixel; float32 blend in ATen's
// association (l0y*(l0x*p00 + l1x*p01) + l1y*(l0x*p10 + l1x*p11)), rounded once to bf16.  ATen's own NHWC kernel runs at
// ~1/7 of the HBM rate on these shapes (measured 1.78 ms per 16-frame batch for ~1 GB of traffic).
__global__ __launch_bounds__(256) void k_upsample_bilinear_nhwc(const uint4* __restrict__ in, uint4* __restrict__ out, int ih, int iw,
                                                                int oh, int ow, int c8, float sh, float sw, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % c8);
  long long r = idx / c8;
  const int x = (int)(r % ow); r /= ow;
  const int y = (int)(r % oh);
  const long long b = r / oh;
  const float fy = sh * (float)y, fx = sw * (float)x;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < ih - 1 ? 1 : 0), x1 = x0 + (x0 < iw - 1 ? 1 : 0);
  const float ly1 = fy - (float)y0, ly0 = 1.f - ly1, lx1 = fx - (float)x0, lx0 = 1.f - lx1;
  const uint4* base = in + (size_t)b * ih * iw * c8 + c;
  const uint4 p00 = base[((size_t)y0 * iw + x0) * c8], p01 = base[((size_t)y0 * iw + x1) * c8];
  const uint4 p10 = base[((size_t)y1 * iw + x0) * c8], p11 = base[((size_t)y1 * iw + x1) * c8];
  const uint32_t a00[4] = {p00.x, p00.y, p00.z, p00.w}, a01[4] = {p01.x, p01.y, p01.z, p01.w};
  const uint32_t a10[4] = {p10.x, p10.y, p10.z, p10.w}, a11[4] = {p11.x, p11.y, p11.z, p11.w};
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float lo = ly0 * (lx0 * bf2f(a00[j] & 0xffffu) + lx1 * bf2f(a01[j] & 0xffffu)) +
                     ly1 * (lx0 * bf2f(a10[j] & 0xffffu) + lx1 * bf2f(a11[j] & 0xffffu));
    const float hi = ly0 * (lx0 * bf2f(a00[j] >> 16) + lx1 * bf2f(a01[j] >> 16)) +
                     ly1 * (lx0 * bf2f(a10[j] >> 16) + lx1 * bf2f(a11[j] >> 16));
    o[j] = f2bf(lo) | (f2bf(hi) << 16);
  }
  out[idx] = make_uint4(o[0], o[1], o[2], o[3]);
}
// float32 variant: one thread = 4 channels (16 B) of one output column in UP_YT consecutive output rows, ATen's association.  The grid runs over
// (span of UP_SPAN quads along an output row, group of UP_YT rows, image): the row taps (fy, y0, y1, ly0, ly1) and the three row bases are uniform per
// workgroup and live in scalar registers (64-bit only there), the column taps and every per-thread offset are 32-bit (IT = int; long long only for rows of
// 2^31 quads and more).  cshift = log2(c4) where c4 is a power of two, else -1 (one 32-bit division).  Same expression as ever, operation for operation:
// sh * (float)y, (int) truncation, the < ih - 1 clamp, 1.f - l, (ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11)) [+ bias].
#define UP_YT 2
#define UP_SPAN 256
template <typename IT, bool BIAS>
VD_DEV void upsample_bilinear_f32_body(const float4* __restrict__ in, const float4* __restrict__ bias, float4* __restrict__ out, int B, int ih, int iw,
                                       int oh, int ow, int c4, int cshift, float sh, float sw) {
  const IT e = (IT)blockIdx.x * UP_SPAN + (IT)threadIdx.x;      // quad index inside the output row
  if (e >= (IT)ow * c4) return;
  int x, c;
  if (cshift >= 0) { x = (int)(e >> cshift); c = (int)e & (c4 - 1); }
  else { x = (int)(e / c4); c = (int)(e - (IT)x * c4); }
  const float fx = sw * (float)x;
  const int x0 = (int)fx;
  const int x1 = x0 + (x0 < iw - 1 ? 1 : 0);
  const float lx1 = fx - (float)x0, lx0 = 1.f - lx1;
  const IT o0 = (IT)x0 * c4 + c, o1 = (IT)x1 * c4 + c;
  float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
  if (BIAS) bb = bias[c];
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    for (int yb = blockIdx.y * UP_YT; yb < oh; yb += gridDim.y * UP_YT) {
      float4 p00[UP_YT], p01[UP_YT], p10[UP_YT], p11[UP_YT];
      float ly0[UP_YT], ly1[UP_YT];
#pragma unroll
      for (int r = 0; r < UP_YT; ++r) {
        const int y = yb + r < oh ? yb + r : oh - 1;            // a row past the end recomputes the last one and is not stored
        const float fy = sh * (float)y;
        const int y0 = __builtin_amdgcn_readfirstlane((int)fy);   // uniform: the row bases below are scalar arithmetic
        const int y1 = y0 + (y0 < ih - 1 ? 1 : 0);
        ly1[r] = fy - (float)y0; ly0[r] = 1.f - ly1[r];
        const float4* r0 = in + ((size_t)b * ih + y0) * iw * c4;
        const float4* r1 = in + ((size_t)b * ih + y1) * iw * c4;
        p00[r] = r0[o0]; p01[r] = r0[o1]; p10[r] = r1[o0]; p11[r] = r1[o1];
      }
#pragma unroll
      for (int r = 0; r < UP_YT; ++r) {
        if (yb + r >= oh) break;
        float4 o;
        o.x = ly0[r] * (lx0 * p00[r].x + lx1 * p01[r].x) + ly1[r] * (lx0 * p10[r].x + lx1 * p11[r].x);
        o.y = ly0[r] * (lx0 * p00[r].y + lx1 * p01[r].y) + ly1[r] * (lx0 * p10[r].y + lx1 * p11[r].y);
        o.z = ly0[r] * (lx0 * p00[r].z + lx1 * p01[r].z) + ly1[r] * (lx0 * p10[r].z + lx1 * p11[r].z);
        o.w = ly0[r] * (lx0 * p00[r].w + lx1 * p01[r].w) + ly1[r] * (lx0 * p10[r].w + lx1 * p11[r].w);
        if (BIAS) { o.x = o.x + bb.x; o.y = o.y + bb.y; o.z = o.z + bb.z; o.w = o.w + bb.w; }
        (out + ((size_t)b * oh + (yb + r)) * ow * c4)[e] = o;
      }
    }
  }
}
template <typename IT>
__global__ __launch_bounds__(UP_SPAN) void k_upsample_bilinear_nhwc_f32(const float4* __restrict__ in, float4* __restrict__ out, int B, int ih, int iw,
                                                                        int oh, int ow, int c4, int cshift, float sh, float sw) {
  upsample_bilinear_f32_body<IT, false>(in, nullptr, out, B, ih, iw, oh, ow, c4, cshift, sh, sw);
}
// ... with the producing convolution's bias added to the interpolated value: the interpolation weights sum to one, so up(conv + b) == up(conv) + b;
// the convolution in front runs without its bias pass.
template <typename IT>
__global__ __launch_bounds__(UP_SPAN) void k_upsample_bilinear_bias_nhwc_f32(const float4* __restrict__ in, const float4* __restrict__ bias,
                                                                             float4* __restrict__ out, int B, int ih, int iw, int oh, int ow, int c4,
                                                                             int cshift, float sh, float sw) {
  upsample_bilinear_f32_body<IT, true>(in, bias, out, B, ih, iw, oh, ow, c4, cshift, sh, sw);
}
static bool launch_upsample_bilinear_f32(hipStream_t s, const float* in, const float* bias, float* out, int B, int ih, int iw, int oh, int ow, int C) {
  if (C % 4 || oh < 2 || ow < 2) return false;
  const int c4 = C / 4;
  const int cshift = (c4 & (c4 - 1)) ? -1 : __builtin_ctz((unsigned)c4);
  const float sh = (float)(ih - 1) / (float)(oh - 1), sw = (float)(iw - 1) / (float)(ow - 1);   // area_pixel_compute_scale, align_corners
  const long long rowq = (long long)ow * c4, inq = (long long)iw * c4;                            // quads per output / input row
  const long long gx = (rowq + UP_SPAN - 1) / UP_SPAN, gy = ((long long)oh + UP_YT - 1) / UP_YT;
  if (gx > 0x7fffffffll) return false;
  const dim3 g((unsigned)gx, (unsigned)(gy < 65535 ? gy : 65535), (unsigned)(B < 65535 ? B : 65535));
  const bool wide = rowq >= (1ll << 31) - UP_SPAN || inq >= (1ll << 31);
  const float4 *i4 = (const float4*)in, *b4 = (const float4*)bias;
  float4* o4 = (float4*)out;
  if (bias) {
    if (wide) hipLaunchKernelGGL(k_upsample_bilinear_bias_nhwc_f32<long long>, g, dim3(UP_SPAN), 0, s, i4, b4, o4, B, ih, iw, oh, ow, c4, cshift, sh, sw);
    else hipLaunchKernelGGL(k_upsample_bilinear_bias_nhwc_f32<int>, g, dim3(UP_SPAN), 0, s, i4, b4, o4, B, ih, iw, oh, ow, c4, cshift, sh, sw);
  } else {
    if (wide) hipLaunchKernelGGL(k_upsample_bilinear_nhwc_f32<long long>, g, dim3(UP_SPAN), 0, s, i4, o4, B, ih, iw, oh, ow, c4, cshift, sh, sw);
    else hipLaunchKernelGGL(k_upsample_bilinear_nhwc_f32<int>, g, dim3(UP_SPAN), 0, s, i4, o4, B, ih, iw, oh, ow, c4, cshift, sh, sw);
  }
  return true;
}
bool vd_launch_upsample_bilinear_nhwc(hipStream_t s, int dtype, const void* in, void* out, int B, int ih, int iw, int oh, int ow, int C) {
  if (dtype == VD3D_DT_F32) return launch_upsample_bilinear_f32(s, (const float*)in, nullptr, (float*)out, B, ih, iw, oh, ow, C);
  if (dtype != VD3D_DT_BF16) return false;
  if (C % 8 || oh < 2 || ow < 2) return false;
  const int c8 = C / 8;
  const long long total = (long long)B * oh * ow * c8;
  const float sh = (float)(ih - 1) / (float)(oh - 1), sw = (float)(iw - 1) / (float)(ow - 1);   // area_pixel_compute_scale, align_corners
  hipLaunchKernelGGL(k_upsample_bilinear_nhwc, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const uint4*)in, (uint4*)out, ih, iw,
                     oh, ow, c8, sh, sw, total);
  return true;
}

// ---- DPT neck / head glue in float32 (round 4): what sits between MIOpen's convolutions in DepthAnythingPreActResidualLayer /
// FeatureFusionLayer / DepthEstimationHead (transformers modeling_depth_anything.py).  PyTorch runs each bias, ReLU and residual sum as its
// own pass over the feature map (bias: a broadcast add behind every MIOpen convolution); at 4K the head-resolution maps are 0.6 - 1.3 GB.
//
// k_bias_act: v = y [+ bias[c]] [+ r1] ; [v = r2 + v] ; [v = max(v, 0)] -> out ; [relu_out = max(v, 0)]   (NHWC, one thread = 4 channels)
//   second convolution of a residual unit: bias + the unit's input (+ the fusion layer's running state) in one pass, and the ReLU'd copy the next
//   unit's first convolution reads; first convolution: bias + ReLU in place.
__global__ __launch_bounds__(256) void k_bias_act(const float4* __restrict__ y, const float4* __restrict__ bias, const float4* __restrict__ r1,
                                                  const float4* __restrict__ r2, int relu, int c4, long long total, float4* __restrict__ out,
                                                  float4* __restrict__ relu_out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  float4 v = y[idx];
  if (bias) { const float4 b = bias[(int)(idx % c4)]; v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
  if (r1) { const float4 r = r1[idx]; v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
  if (r2) { const float4 r = r2[idx]; v.x = r.x + v.x; v.y = r.y + v.y; v.z = r.z + v.z; v.w = r.w + v.w; }
  if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  out[idx] = v;
  if (relu_out) relu_out[idx] = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}
bool vd_launch_bias_act_f32(hipStream_t s, const float* y, const float* bias, const float* r1, const float* r2, int relu, long long n_pix, int C,
                            float* out, float* relu_out) {
  if (C % 4 || n_pix < 1) return false;
  const long long total = n_pix * (C / 4);
  hipLaunchKernelGGL(k_bias_act, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float4*)y, (const float4*)bias, (const float4*)r1,
                     (const float4*)r2, relu, C / 4, total, (float4*)out, (float4*)relu_out);
  return true;
}

bool vd_launch_upsample_bilinear_bias_nhwc_f32(hipStream_t s, const float* in, const float* bias, float* out, int B, int ih, int iw, int oh, int ow, int C) {
  if (!bias) return false;
  return launch_upsample_bilinear_f32(s, in, bias, out, B, ih, iw, oh, ow, C);
}

// k_head_tail: everything behind the head's second convolution -- its bias, ReLU, the 1x1 convolution to ONE channel (a C-term dot product per
// pixel), its bias, the final activation and max_depth -- in one pass: reads the C-channel map once, writes one float per pixel (PyTorch: bias r+w, ReLU r+w,
// MIOpen 1x1 r, bias, activation, scale).  LPP = C / 4 adjacent lanes share a pixel (coalesced 16-byte loads), partial dot products meet in a butterfly.
// ACT (VD3D_HEAD_ACT_*) is the head's last activation: 0 = ReLU (the relative Depth-Anything heads, DPT), 1 = torch.sigmoid (the metric Depth-Anything heads:
// vd_sigmoid_torch, the values torch's CPU kernel gives); the activation and the multiplication by scale are two float32 roundings, as in the module graph.
// A template parameter: the ReLU instantiations hold no trace of the other branch.  NaN: fmaxf(NaN, 0) is 0, so the ReLU tail has always turned a NaN in y into
// a finite value (both of its ReLUs do); the sigmoid tail keeps a NaN alive through the inner ReLU -- its pixel, and no other, comes out NaN, as torch's graph
// gives it -- and is the same arithmetic, bit for bit, on every other input.
template <int ACT>
VD_DEV float head_tail_relu(float x) {
  if constexpr (ACT == 1) return x != x ? x : fmaxf(x, 0.f);
  else return fmaxf(x, 0.f);
}
template <int LPP, int ACT>
__global__ __launch_bounds__(256) void k_head_tail(const float4* __restrict__ y, const float4* __restrict__ b2, const float4* __restrict__ w3, float b3,
                                                   float scale, long long n_pix, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pix = idx / LPP;
  const int l = (int)(idx % LPP);
  float acc = 0.f;
  if (pix < n_pix) {
    const float4 v = y[idx], b = b2[l], w = w3[l];
    acc = head_tail_relu<ACT>(v.x + b.x) * w.x;
    acc = vd_fma(head_tail_relu<ACT>(v.y + b.y), w.y, acc);
    acc = vd_fma(head_tail_relu<ACT>(v.z + b.z), w.z, acc);
    acc = vd_fma(head_tail_relu<ACT>(v.w + b.w), w.w, acc);
  }
#pragma unroll
  for (int off = LPP / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (l == 0 && pix < n_pix) {
    if constexpr (ACT == 1) out[pix] = vd_sigmoid_torch(acc + b3) * scale;
    else out[pix] = fmaxf(acc + b3, 0.f) * scale;
  }
}
template <int ACT>
static bool launch_head_tail(hipStream_t s, const float4* yy, const float4* bb, const float4* ww, float b3, float scale, long long n_pix, int C, float* out) {
  const long long total = n_pix * (C / 4);
  const dim3 g((unsigned)((total + 255) / 256)), b(256);
  switch (C) {
    case 16: hipLaunchKernelGGL((k_head_tail<4, ACT>), g, b, 0, s, yy, bb, ww, b3, scale, n_pix, out); return true;
    case 32: hipLaunchKernelGGL((k_head_tail<8, ACT>), g, b, 0, s, yy, bb, ww, b3, scale, n_pix, out); return true;
    case 64: hipLaunchKernelGGL((k_head_tail<16, ACT>), g, b, 0, s, yy, bb, ww, b3, scale, n_pix, out); return true;
    default: return false;
  }
}
// act: 0 = ReLU, 1 = sigmoid (the caller has checked it).  false = nothing launched: C not in {16, 32, 64}, n_pix < 1, a grid past 2^31 - 1 workgroups, or
// y / b2 / w3 not 16-byte aligned (the kernel reads them as float4) or out not 4-byte aligned.
bool vd_launch_head_tail_f32(hipStream_t s, const float* y, const float* b2, const float* w3, float b3, float scale, long long n_pix, int C, int act, float* out) {
  if (n_pix < 1 || (C != 16 && C != 32 && C != 64) || (n_pix * (C / 4) + 255) / 256 > 0x7fffffffLL) return false;
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(b2) | reinterpret_cast<uintptr_t>(w3)) & 15) || (reinterpret_cast<uintptr_t>(out) & 3)) return false;
  const float4 *yy = (const float4*)y, *bb = (const float4*)b2, *ww = (const float4*)w3;
  return act == 1 ? launch_head_tail<1>(s, yy, bb, ww, b3, scale, n_pix, C, out) : launch_head_tail<0>(s, yy, bb, ww, b3, scale, n_pix, C, out);
}

// k_depth_to_space_bias: the scatter half of DPT's reassemble-stage ConvTranspose2d(C, C, kernel_size=s, stride=s) -- kernel == stride, so the layer is a GEMM
// Y[p][(i, j, c)] (vd3d_gemm_x3) whose rows land in disjoint s x s output windows.  y [P = B*H*W][s][s][C] -> out NHWC [B][H*s][W*s][C], + bias[c]: an exact
// copy and one float32 add.  One thread = 4 channels (16 B) of one OUTPUT pixel: stores are dense rows, loads are runs of s * C floats (one window row).
__global__ __launch_bounds__(256) void k_depth_to_space_bias(const float4* __restrict__ y, const float4* __restrict__ bias, int H, int W, int s, int c4,
                                                             long long total, float4* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % c4);
  long long r = idx / c4;
  const int ow = W * s, oh = H * s;
  const int ox = (int)(r % ow); r /= ow;
  const int oy = (int)(r % oh);
  const long long b = r / oh;
  const int py = oy / s, i = oy - py * s, px = ox / s, j = ox - px * s;
  const long long p = (b * H + py) * W + px;
  float4 v = y[((p * s + i) * s + j) * c4 + c];
  if (bias) { const float4 bb = bias[c]; v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w; }
  out[idx] = v;
}
bool vd_launch_depth_to_space_bias_f32(hipStream_t s, const float* y, const float* bias, int B, int H, int W, int f, int C, float* out) {
  if (C % 4 || B < 1 || H < 1 || W < 1 || f < 1) return false;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(out)) & 15) return false;
  const long long total = (long long)B * H * f * W * f * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  hipLaunchKernelGGL(k_depth_to_space_bias, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float4*)y, (const float4*)bias, H, W, f, C / 4,
                     total, (float4*)out);
  return true;
}

// k_patchify: the gather half of a ViT patch embedding (Conv2d(3, C, kernel_size=p, stride=p)) run as a GEMM -- kernel == stride, so every patch is one row:
// x NHWC [B][th][tw][3] (what vd3d_depth_preprocess writes) -> rows [B * gh * gw][Kp], gh = th / p, gw = tw / p (the convolution drops a remainder), column
// (c * p + ky) * p + kx = x[b][gy p + ky][gx p + kx][c] (F.unfold's order = the flattened weight [C][3][p][p]); the columns from 3 p^2 to Kp (3 p^2 rounded
// up to the GEMM's K unit of 16) are written as zeros.  Exact copies.  One thread = 4 consecutive columns (one 16-byte store).
__global__ __launch_bounds__(256) void k_patchify(const float* __restrict__ x, int th, int tw, int p, int gh, int gw, int kp4, long long total,
                                                  float4* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k4 = (int)(idx % kp4);
  long long r = idx / kp4;
  const int gx = (int)(r % gw); r /= gw;
  const int gy = (int)(r % gh);
  const long long b = r / gh;
  const int pp = p * p, K = 3 * pp;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = k4 * 4 + e;
    v[e] = 0.f;
    if (k < K) {
      const int c = k / pp, rem = k - c * pp, ky = rem / p, kx = rem - ky * p;
      v[e] = x[((b * th + (gy * p + ky)) * tw + (gx * p + kx)) * 3 + c];
    }
  }
  out[idx] = float4{v[0], v[1], v[2], v[3]};
}
bool vd_launch_patchify_f32(hipStream_t s, const float* x, int B, int th, int tw, int p, float* out) {
  if (B < 1 || p < 1 || p > 64 || th < p || tw < p) return false;
  if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(out) & 15)) return false;
  const int gh = th / p, gw = tw / p, kp = (3 * p * p + 15) / 16 * 16;
  const long long total = (long long)B * gh * gw * (kp / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  hipLaunchKernelGGL(k_patchify, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, th, tw, p, gh, gw, kp / 4, total, (float4*)out);
  return true;
}
