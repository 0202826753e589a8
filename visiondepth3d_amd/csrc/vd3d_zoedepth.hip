// vd3d_zoedepth.hip -- the four kernels around ZoeDepth (ZoeDepthForDepthEstimation) in DepthPipe: the image processor's padded front end, its un-padding
// post-process, and the two kernels of the metric bin head.  visiondepth3d_amd/zoedepth.py states all four (preprocess_statement, post_statement,
// attractor_statement, bins_statement); tests/test_hip_zoedepth_kernels.py holds the kernels to them.  Every map is float32 NHWC.
//
// "Bilinear" below is F.interpolate(mode="bilinear", align_corners=True) as ATen evaluates it: scale = float(in - 1) / float(out - 1) (0 for out == 1, divided
// on the host), src = scale d, i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1 and
// out = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), every operation rounded on its own (-ffp-contract=off); a zero-weight tap is still multiplied in.
//
// k_zoe_preprocess: uint8 BGR [B][H][W][3] -> pixel_values [B][th][tw][3] (R, G, B).  The processor rescales first (a 256-entry table of the byte, built by the
//                   caller with the class's own rescale and staged in LDS), pads by reflection (folded into the gather index: no padded image exists), resizes
//                   bilinearly and normalises last, (v - mean) / std.  One thread = one output pixel.
// k_zoe_post:       prediction [B][th][tw] -> [B][H][W]: ATen's bicubic (A = -0.75, align_corners=False, clamped tap indices) on the (H + 2 ph) x (W + 2 pw) grid,
//                   evaluated only at the rows and columns that survive the crop.  One thread = one output pixel.
// k_zoe_attractor:  ZoeDepthAttractorLayerUnnormed behind its MLP: new bins = c + (sum_i dx_i / (1 + 300 dx_i dx_i)) [/ nA], c the bilinear sample of the previous
//                   bins, dx_i = a_i - c, summed in ascending i from zero in the module's operation order.  One thread = four bins of one pixel.
// k_zoe_bins:       the conditional log-binomial tail: per pixel the two-layer MLP (first layer = W1_last . last + bilinear(W1_e . e) + b1, exact GELU, four
//                   outputs, softplus), p and the temperature, the log-binomial logits over the bins, a max-subtracted softmax and the expectation against the
//                   bilinearly sampled bins.  No per-bin tensor is written.  The MLP is float32 (fused multiply-adds); softplus, p, the temperature and the logits are
//                   float64 (see the kernel), the exponential and the sums float32.  One thread = one pixel; the weights are read at wave-uniform addresses.
#include "vd3d_dev.h"
#include "vd3d_cubic.h"
#include "vd3d_kernels.h"

struct zoe_tap { int i0, i1; float l0, l1; };
VD_DEV zoe_tap zoe_linear_tap(int d, int in, float scale) {
  zoe_tap t;
  const float src = scale * (float)d;
  int i0 = (int)src;
  i0 = i0 < in - 1 ? i0 : in - 1;
  t.i0 = i0; t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  t.l1 = src - (float)i0; t.l0 = 1.f - t.l1;
  return t;
}
VD_DEV float zoe_blend(const zoe_tap& ty, const zoe_tap& tx, float v00, float v01, float v10, float v11) {
  const float top = tx.l0 * v00 + tx.l1 * v01, bot = tx.l0 * v10 + tx.l1 * v11;
  return ty.l0 * top + ty.l1 * bot;
}
VD_DEV float4 zoe_blend4(const zoe_tap& ty, const zoe_tap& tx, float4 a, float4 b, float4 c, float4 d) {
  return float4{zoe_blend(ty, tx, a.x, b.x, c.x, d.x), zoe_blend(ty, tx, a.y, b.y, c.y, d.y), zoe_blend(ty, tx, a.z, b.z, c.z, d.z), zoe_blend(ty, tx, a.w, b.w, c.w, d.w)};
}
static inline float zoe_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
// index into the unpadded axis of length n for index p of the axis padded by `pad` on both sides (np.pad mode="reflect"; pad < n)
VD_DEV int zoe_reflect(int p, int pad, int n) {
  const int i = p - pad;
  return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
}

struct zoe_norm { float m[3], s[3]; };

__global__ __launch_bounds__(256) void k_zoe_preprocess(const uint8_t* __restrict__ frames, const float* __restrict__ table, int H, int W, int ph, int pw, int th, int tw,
                                                        float sy, float sx, zoe_norm nm, long long total, float* __restrict__ out) {
  __shared__ float tab[256];
  tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % tw);
  const long long r = idx / tw;
  const int y = (int)(r % th);
  const long long b = r / th;
  const zoe_tap ty = zoe_linear_tap(y, H + 2 * ph, sy), tx = zoe_linear_tap(x, W + 2 * pw, sx);
  const uint8_t* r0 = frames + (b * H + zoe_reflect(ty.i0, ph, H)) * (long long)W * 3;
  const uint8_t* r1 = frames + (b * H + zoe_reflect(ty.i1, ph, H)) * (long long)W * 3;
  const int a = zoe_reflect(tx.i0, pw, W) * 3, c = zoe_reflect(tx.i1, pw, W) * 3;
  float* o = out + idx * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {   // channel ch (R, G, B) reads byte 2 - ch of the BGR pixel
    const float v = zoe_blend(ty, tx, tab[r0[a + 2 - ch]], tab[r0[c + 2 - ch]], tab[r1[a + 2 - ch]], tab[r1[c + 2 - ch]]);
    o[ch] = (v - nm.m[ch]) / nm.s[ch];
  }
}

// false = nothing launched (the caller has checked the shapes): a grid past 2^31 - 1 workgroups
bool vd_launch_zoedepth_preprocess_u8(hipStream_t s, const uint8_t* frames, const float* table, int B, int H, int W, int ph, int pw, int th, int tw, const float mean[3],
                                      const float std[3], float* out) {
  const long long total = (long long)B * th * tw;
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  zoe_norm nm;
  for (int c = 0; c < 3; ++c) { nm.m[c] = mean[c]; nm.s[c] = std[c]; }
  hipLaunchKernelGGL(k_zoe_preprocess, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, table, H, W, ph, pw, th, tw, zoe_scale(H + 2 * ph, th),
                     zoe_scale(W + 2 * pw, tw), nm, total, out);
  return true;
}

// ATen's bicubic taps of one axis (align_corners=False, no scale factor given): src = scale (d + 0.5) - 0.5 with scale = float(in) / out, not clamped; the four tap
// indices floor(src) - 1 .. + 2 are clamped into the axis
struct zoe_cubic { int i[4]; float c[4]; };
VD_DEV zoe_cubic zoe_cubic_tap(int d, int in, float scale) {
  zoe_cubic t;
  const float src = scale * ((float)d + 0.5f) - 0.5f;
  const float f = floorf(src);
  const int i0 = (int)f;
  cubic_coeffs(src - f, t.c);
#pragma unroll
  for (int k = 0; k < 4; ++k) { const int i = i0 - 1 + k; t.i[k] = i < 0 ? 0 : (i > in - 1 ? in - 1 : i); }
  return t;
}

__global__ __launch_bounds__(256) void k_zoe_post(const float* __restrict__ pred, int th, int tw, int H, int W, int ph, int pw, float sy, float sx, long long total,
                                                  float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W);
  const long long r = idx / W;
  const int y = (int)(r % H);
  const long long b = r / H;
  const zoe_cubic ty = zoe_cubic_tap(y + ph, th, sy), tx = zoe_cubic_tap(x + pw, tw, sx);
  const float* p = pred + b * (long long)th * tw;
  float rows[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* row = p + (long long)ty.i[i] * tw;
    rows[i] = row[tx.i[0]] * tx.c[0] + row[tx.i[1]] * tx.c[1] + row[tx.i[2]] * tx.c[2] + row[tx.i[3]] * tx.c[3];
  }
  out[idx] = rows[0] * ty.c[0] + rows[1] * ty.c[1] + rows[2] * ty.c[2] + rows[3] * ty.c[3];
}

bool vd_launch_zoedepth_post_f32(hipStream_t s, const float* pred, int B, int th, int tw, int H, int W, int ph, int pw, float* out) {
  const long long total = (long long)B * H * W;
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  hipLaunchKernelGGL(k_zoe_post, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pred, th, tw, H, W, ph, pw, (float)th / (float)(H + 2 * ph),
                     (float)tw / (float)(W + 2 * pw), total, out);
  return true;
}

template <bool MEAN>
__global__ __launch_bounds__(256) void k_zoe_attractor(const float* __restrict__ att, const float* __restrict__ prev, int h, int w, int hp, int wp, int nA, int nb,
                                                       float sy, float sx, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int q = nb >> 2;
  const int j = (int)(idx % q) * 4;
  const long long pix = idx / q;
  const int x = (int)(pix % w);
  const long long r = pix / w;
  const int y = (int)(r % h);
  const long long b = r / h;
  const zoe_tap ty = zoe_linear_tap(y, hp, sy), tx = zoe_linear_tap(x, wp, sx);
  const float* pb = prev + b * (long long)hp * wp * nb + j;
  const float4 v00 = *reinterpret_cast<const float4*>(pb + ((long long)ty.i0 * wp + tx.i0) * nb), v01 = *reinterpret_cast<const float4*>(pb + ((long long)ty.i0 * wp + tx.i1) * nb);
  const float4 v10 = *reinterpret_cast<const float4*>(pb + ((long long)ty.i1 * wp + tx.i0) * nb), v11 = *reinterpret_cast<const float4*>(pb + ((long long)ty.i1 * wp + tx.i1) * nb);
  const float4 c4 = zoe_blend4(ty, tx, v00, v01, v10, v11);
  const float c[4] = {c4.x, c4.y, c4.z, c4.w};
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* a = att + pix * nA;
  for (int i = 0; i < nA; ++i) {
    const float ai = a[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // inv_attractor: dx.div(1 + alpha * dx.pow(2)), alpha = 300
      const float dx = ai - c[e];
      acc[e] = acc[e] + dx / (1.f + 300.f * (dx * dx));
    }
  }
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = c[e] + (MEAN ? acc[e] / (float)nA : acc[e]);
  *reinterpret_cast<float4*>(out + pix * nb + j) = float4{o[0], o[1], o[2], o[3]};
}

bool vd_launch_zoedepth_attractor_f32(hipStream_t s, const float* att, const float* prev, int B, int h, int w, int hp, int wp, int nA, int nb, int mean, float* out) {
  const long long total = (long long)B * h * w * (nb / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  const dim3 g((unsigned)((total + 255) / 256)), blk(256);
  const float sy = zoe_scale(hp, h), sx = zoe_scale(wp, w);
  if (mean) hipLaunchKernelGGL(k_zoe_attractor<true>, g, blk, 0, s, att, prev, h, w, hp, wp, nA, nb, sy, sx, total, out);
  else hipLaunchKernelGGL(k_zoe_attractor<false>, g, blk, 0, s, att, prev, h, w, hp, wp, nA, nb, sy, sx, total, out);
  return true;
}

VD_DEV double zoe_softplus64(double x) { return x > 20.0 ? x : log1p(exp(x)); }   // torch's softplus, beta 1, threshold 20
VD_DEV float zoe_gelu(float x) { return (x * 0.5f) * (1.f + erff(x * 0.70710678118654752440f)); }

#define ZOE_LAST 32   // channels of the relative head's feature map (config.num_relative_features)
__global__ __launch_bounds__(256) void k_zoe_bins(const float* __restrict__ last, const float* __restrict__ rel, const float* __restrict__ wrel, const float* __restrict__ P,
                                                  const float* __restrict__ bins, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                  const float* __restrict__ b2, const float* __restrict__ table, double min_temp, double temp_range, int H, int W, int hc,
                                                  int wc, int Ch, int nb, float sy, float sx, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W);
  const long long r = idx / W;
  const int y = (int)(r % H);
  const long long b = r / H;
  const zoe_tap ty = zoe_linear_tap(y, hc, sy), tx = zoe_linear_tap(x, wc, sx);
  const long long o00 = (b * hc + ty.i0) * (long long)wc + tx.i0, o01 = (b * hc + ty.i0) * (long long)wc + tx.i1;
  const long long o10 = (b * hc + ty.i1) * (long long)wc + tx.i0, o11 = (b * hc + ty.i1) * (long long)wc + tx.i1;
  float l[ZOE_LAST];
#pragma unroll
  for (int k = 0; k < ZOE_LAST; k += 4) {
    const float4 v = *reinterpret_cast<const float4*>(last + idx * ZOE_LAST + k);
    l[k] = v.x; l[k + 1] = v.y; l[k + 2] = v.z; l[k + 3] = v.w;
  }
  const float rv = rel ? rel[idx] : 0.f;
  float o[4] = {b2[0], b2[1], b2[2], b2[3]};
  for (int c = 0; c < Ch; c += 4) {
    const float4 pe = zoe_blend4(ty, tx, *reinterpret_cast<const float4*>(P + o00 * Ch + c), *reinterpret_cast<const float4*>(P + o01 * Ch + c),
                                 *reinterpret_cast<const float4*>(P + o10 * Ch + c), *reinterpret_cast<const float4*>(P + o11 * Ch + c));
    const float pv[4] = {pe.x, pe.y, pe.z, pe.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* wr = w1 + (long long)(c + e) * ZOE_LAST;
      float hsum = 0.f;
#pragma unroll
      for (int k = 0; k < ZOE_LAST; ++k) hsum = vd_fma(wr[k], l[k], hsum);
      if (rel) hsum = vd_fma(wrel[c + e], rv, hsum);
      const float g = zoe_gelu((hsum + pv[e]) + b1[c + e]);
#pragma unroll
      for (int m = 0; m < 4; ++m) o[m] = vd_fma(w2[(long long)m * Ch + c + e], g, o[m]);
    }
  }
  // Behind the MLP the arithmetic is float64 up to the exponent: the logits reach (nb - 1) |log 1e-4| and are divided by a temperature as small as min_temp, so a
  // float32 logit would carry its rounding, times 1 / temperature, straight into the softmax weights.  The exponential itself, of the max-subtracted logit, and the two
  // sums are float32.
  double sp[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) sp[m] = zoe_softplus64((double)o[m]) + 1e-4;
  const double p = sp[0] / (sp[0] + sp[1]);
  const double inv_temp = 1.0 / (temp_range * (sp[2] / (sp[2] + sp[3])) + min_temp);
  const double q = 1.0 - p;
  const double lp = log(p < 1e-4 ? 1e-4 : (p > 1.0 ? 1.0 : p)), lq = log(q < 1e-4 ? 1e-4 : (q > 1.0 ? 1.0 : q));   // (NaN passes both comparisons and stays NaN)
  double mx = -INFINITY;
  for (int k = 0; k < nb; ++k) {
    const double yk = (((double)table[k] + (double)k * lp) + (double)(nb - 1 - k) * lq) * inv_temp;
    mx = yk > mx ? yk : mx;   // (a NaN logit leaves the maximum alone and reaches the sums below)
  }
  float den = 0.f, num = 0.f;
  for (int k = 0; k < nb; k += 4) {
    const float4 c4 = zoe_blend4(ty, tx, *reinterpret_cast<const float4*>(bins + o00 * nb + k), *reinterpret_cast<const float4*>(bins + o01 * nb + k),
                                 *reinterpret_cast<const float4*>(bins + o10 * nb + k), *reinterpret_cast<const float4*>(bins + o11 * nb + k));
    const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double yk = (((double)table[k + e] + (double)(k + e) * lp) + (double)(nb - 1 - k - e) * lq) * inv_temp;
      const float w = expf((float)(yk - mx));
      den += w;
      num = vd_fma(w, cv[e], num);
    }
  }
  out[idx] = num / den;
}

bool vd_launch_zoedepth_bins_f32(hipStream_t s, const float* last, const float* rel, const float* wrel, const float* P, const float* bins, const float* w1, const float* b1,
                                 const float* w2, const float* b2, const float* table, double min_temp, double temp_range, int B, int H, int W, int hc, int wc, int Ch, int nb,
                                 float* out) {
  const long long total = (long long)B * H * W;
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  hipLaunchKernelGGL(k_zoe_bins, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, last, rel, wrel, P, bins, w1, b1, w2, b2, table, min_temp, temp_range, H, W, hc, wc,
                     Ch, nb, zoe_scale(hc, H), zoe_scale(wc, W), total, out);
  return true;
}
