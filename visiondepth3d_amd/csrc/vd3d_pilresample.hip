// vd3d_pilresample.hip -- Pillow's 8-bit bicubic resampler (ImagingResample: what Image.resize(size, Image.BICUBIC) runs on an RGB image), bit for bit, and
// the depth network's input built on it: DepthPipe(front_end="pil").  The reference hands its depth pipeline PIL images (core/render_depth.py:1113-1116,
// 1815-1821) and the Hugging Face image processor resizes them with Pillow again, so the network sees bytes that were rounded after the horizontal and
// again after the vertical pass.  visiondepth3d_amd/pil_resample.py states the operator; this file is its device form and gives the same bytes.
//
// Per axis the host builds, in IEEE double and Pillow's order (precompute_coeffs, normalize_coeffs_8bpc), the first tap, the tap count and the 22-bit
// fixed-point coefficients of every output index; a pass is acc = 2^21 + sum(byte * k) in int32, clamp(acc >> 22, 0, 255).  An axis that keeps its size
// gets the identity table (one tap of 2^22: (2^21 + 2^22 p) >> 22 == p), so one kernel covers both passes, one pass and the copy.  No float touches a pixel.
//
// k_pil_resample: a workgroup owns PR_SX output columns of a band of `by` output rows.  The band's input rows go through LDS in chunks of PR_CH (aligned
// dwords, the next chunk in flight: the fetch of k_depth_prep_strip), are filtered horizontally four taps per step (three dwords, v_alignbyte to the
// byte phase, twelve 24-bit multiply-adds, one 16-byte read of coefficients) and kept as packed bytes (c0 | c1 << 8 | c2 << 16: Pillow's temporary
// image); the vertical pass reads one dword per tap.  Coefficient rows are zero-padded to a multiple of four taps: a padded tap adds 0 whatever byte
// stands behind it.  Epilogues: uint8 in the input's channel order, or BGR -> RGB through the 3 x 256 table of the image processor's rescale and
// normalise, float32 or bf16 (round to nearest even), NHWC.  40 960 bytes of static LDS with the table, 37 888 without: four workgroups per CU.
#include <cmath>
#include <vector>

#include "vd3d_dev.h"
#include "vd3d_kernels.h"

#define PR_SX 32       // output columns of a workgroup
#define PR_BY 32       // output rows of a band at most; the launcher halves it until the band's input rows fit PR_HROWS
#define PR_HROWS 160   // filtered input rows per band
#define PR_CH 16       // input rows per chunk
#define PR_ROWB 640    // bytes of one input row of a strip at most
#define PR_RS 168      // dwords per staged row: PR_ROWB + 3 bytes of phase, 9 bytes of padded taps, the look-ahead dword
#define PR_NLD 11      // dwords per lane and chunk: 16 lanes x 11 >= PR_RS

static_assert(VD_PIL_KMAX % 4 == 0, "coefficient rows are read four taps at a time");
static_assert(16 * PR_NLD >= PR_RS && (PR_ROWB + 3 + 9) / 4 + 2 <= PR_RS, "staged row");

VD_DEV int pr_clip8(int acc) {
  const int v = acc >> 22;   // arithmetic
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
VD_DEV uint16_t pr_bf16(float f) {   // round to nearest even, finite inputs
  const uint32_t b = __float_as_uint(f);
  return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}

// tab_w / tab_h: [n] first tap, [n] tap count, [n][VD_PIL_KMAX] coefficients of the axis (n = w / h).  EPI 0: uint8 [B][h][w][3]; 1: float32, 2: bf16 NHWC
template <int EPI>
__global__ __launch_bounds__(256) void k_pil_resample(const uint8_t* __restrict__ frames, int H, int W, int h, int w, const int* __restrict__ tab_w,
                                                      const int* __restrict__ tab_h, int by, const float* __restrict__ lut, void* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) int kx[PR_SX * VD_PIL_KMAX];
  __shared__ int ky[PR_BY * VD_PIL_KMAX];
  __shared__ int x0s[2 * PR_SX], y0s[2 * PR_BY];
  __shared__ uint32_t hb[PR_HROWS * PR_SX];   // [row][column] packed bytes
  __shared__ uint32_t tile[PR_CH * PR_RS];
  __shared__ float slut[EPI ? 768 : 1];
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * PR_SX, oy0 = blockIdx.y * by, b = blockIdx.z;
  const int nx = min(PR_SX, w - ox0), ny = min(by, h - oy0);
  for (int t = tid; t < PR_SX * VD_PIL_KMAX; t += 256) {
    const int o = t / VD_PIL_KMAX;
    kx[t] = o < nx ? tab_w[2 * w + (ox0 + o) * VD_PIL_KMAX + (t - o * VD_PIL_KMAX)] : 0;
  }
  for (int t = tid; t < by * VD_PIL_KMAX; t += 256) {
    const int o = t / VD_PIL_KMAX;
    ky[t] = o < ny ? tab_h[2 * h + (oy0 + o) * VD_PIL_KMAX + (t - o * VD_PIL_KMAX)] : 0;
  }
  if (tid < PR_SX) {
    x0s[tid] = tid < nx ? tab_w[ox0 + tid] : 0; x0s[PR_SX + tid] = tid < nx ? tab_w[w + ox0 + tid] : 0;
  } else if (tid >= 64 && tid < 64 + by) {
    const int t = tid - 64;
    y0s[t] = t < ny ? tab_h[oy0 + t] : 0; y0s[PR_BY + t] = t < ny ? tab_h[h + oy0 + t] : 0;
  }
  if (EPI)
    for (int t = tid; t < 768; t += 256) slut[t] = lut[t];
  __syncthreads();
  const int c_lo = x0s[0], c_hi = x0s[nx - 1] + x0s[PR_SX + nx - 1];   // [c_lo, c_hi) input columns: first taps never decrease along an axis
  const int r_lo = y0s[0], r_hi = y0s[ny - 1] + y0s[PR_BY + ny - 1];
  const int ncol = min(c_hi - c_lo, PR_ROWB / 3), nrow = min(r_hi - r_lo, PR_HROWS);   // the launcher admits no geometry past either bound
  const int rowbytes = ncol * 3;
  const uint8_t* src = frames + (size_t)b * H * W * 3;
  const int nch = (nrow + PR_CH - 1) / PR_CH;
  const int lr = tid >> 4, ll = tid & 15;
  uint32_t regs[PR_NLD];
  auto fetch = [&](int ch) {
    const int r = ch * PR_CH + lr;
    const uint8_t* g = src + ((size_t)(r_lo + (r < nrow ? r : nrow - 1)) * W + c_lo) * 3;
    const int ph = (int)((uintptr_t)g & 3);
    const uint32_t* gp = reinterpret_cast<const uint32_t*>(g - ph);
    const int ndw = (ph + rowbytes + 3) >> 2;        // every dword fetched holds at least one byte of the row
#pragma unroll
    for (int k = 0; k < PR_NLD; ++k) regs[k] = (ll + 16 * k < ndw) ? gp[ll + 16 * k] : 0u;
  };
  fetch(0);
  for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
    for (int k = 0; k < PR_NLD; ++k)
      if (ll + 16 * k < PR_RS) tile[lr * PR_RS + ll + 16 * k] = regs[k];
    __syncthreads();
    if (ch + 1 < nch) fetch(ch + 1);
    // horizontal pass: (input row, output column) tasks, three channels each
#pragma unroll
    for (int t = tid; t < PR_CH * PR_SX; t += 256) {
      const int rr = t >> 5, ox = t & (PR_SX - 1);
      const int r = ch * PR_CH + rr;
      if (r >= nrow) continue;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      if (ox < nx) {
        const int n4 = (x0s[PR_SX + ox] + 3) >> 2;
        const uint32_t ph = ((uint32_t)(uintptr_t)src + ((uint32_t)(r_lo + r) * (uint32_t)W + (uint32_t)c_lo) * 3u) & 3u;   // the low two bits suffice
        const uint32_t start = ph + (uint32_t)(x0s[ox] - c_lo) * 3u;
        const uint32_t sh = start & 3u;
        const uint32_t* row = tile + rr * PR_RS + (start >> 2);
        const int4* k4 = reinterpret_cast<const int4*>(kx + ox * VD_PIL_KMAX);
        uint32_t lo = row[0];
        for (int g = 0; g < n4; ++g) {
          const uint32_t d1 = row[3 * g + 1], d2 = row[3 * g + 2], d3 = row[3 * g + 3];
          const uint32_t u0 = __builtin_amdgcn_alignbyte(d1, lo, sh), u1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                         u2 = __builtin_amdgcn_alignbyte(d3, d2, sh);   // bytes 0 1 2 0 | 1 2 0 1 | 2 0 1 2 (channel) of taps 4g .. 4g + 3
          lo = d3;
          const int4 k = k4[g];
          s0 += __mul24((int)(u0 & 0xffu), k.x);         s1 += __mul24((int)((u0 >> 8) & 0xffu), k.x);  s2 += __mul24((int)((u0 >> 16) & 0xffu), k.x);
          s0 += __mul24((int)(u0 >> 24), k.y);           s1 += __mul24((int)(u1 & 0xffu), k.y);         s2 += __mul24((int)((u1 >> 8) & 0xffu), k.y);
          s0 += __mul24((int)((u1 >> 16) & 0xffu), k.z); s1 += __mul24((int)(u1 >> 24), k.z);           s2 += __mul24((int)(u2 & 0xffu), k.z);
          s0 += __mul24((int)((u2 >> 8) & 0xffu), k.w);  s1 += __mul24((int)((u2 >> 16) & 0xffu), k.w); s2 += __mul24((int)(u2 >> 24), k.w);
        }
      }
      hb[r * PR_SX + ox] = (uint32_t)pr_clip8(s0) | ((uint32_t)pr_clip8(s1) << 8) | ((uint32_t)pr_clip8(s2) << 16);
    }
    __syncthreads();
  }
  for (int t = tid; t < ny * PR_SX; t += 256) {
    const int oy = t >> 5, ox = t & (PR_SX - 1);
    if (ox >= nx) continue;
    const int rb = y0s[oy] - r_lo, n = min(y0s[PR_BY + oy], nrow - rb);
    const int* k = ky + oy * VD_PIL_KMAX;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int j = 0; j < n; ++j) {
      const uint32_t p = hb[(rb + j) * PR_SX + ox];
      const int kj = k[j];
      s0 += __mul24((int)(p & 0xffu), kj); s1 += __mul24((int)((p >> 8) & 0xffu), kj); s2 += __mul24((int)((p >> 16) & 0xffu), kj);
    }
    const int v0 = pr_clip8(s0), v1 = pr_clip8(s1), v2 = pr_clip8(s2);
    const size_t e = (((size_t)b * h + (oy0 + oy)) * w + (ox0 + ox)) * 3;
    if (EPI == 0) {
      uint8_t* o = reinterpret_cast<uint8_t*>(out) + e;
      o[0] = (uint8_t)v0; o[1] = (uint8_t)v1; o[2] = (uint8_t)v2;
    } else if (EPI == 1) {   // BGR bytes -> RGB values
      float* o = reinterpret_cast<float*>(out) + e;
      o[0] = slut[v2]; o[1] = slut[256 + v1]; o[2] = slut[512 + v0];
    } else {
      uint16_t* o = reinterpret_cast<uint16_t*>(out) + e;
      o[0] = pr_bf16(slut[v2]); o[1] = pr_bf16(slut[256 + v1]); o[2] = pr_bf16(slut[512 + v0]);
    }
  }
}

// ---- host: the tables ----------------------------------------------------------------------------------------------------------------------------
static double pr_cubic(double x) {   // Pillow's bicubic_filter, a = -0.5
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// 0 = built (a->dev holds the table), 1 = outside the kernel's plan (a->dev stays NULL: the caller answers "unsupported" for this geometry from then on),
// -1 = a HIP call failed (*herr).  The library is compiled with -ffp-contract=off: no step below contracts into an FMA.
int vd_pil_axis_build(vd_pil_axis* a, int n_in, int n_out, hipError_t* herr) {
  *a = vd_pil_axis();
  a->n_in = n_in; a->n_out = n_out;
  std::vector<int> tab((size_t)n_out * (2 + VD_PIL_KMAX), 0);
  int* xmin_v = tab.data();
  int* cnt_v = xmin_v + n_out;
  int* k_v = cnt_v + n_out;
  bool fits = true;
  if (n_in == n_out) {
    for (int xx = 0; xx < n_out; ++xx) { xmin_v[xx] = xx; cnt_v[xx] = 1; k_v[(size_t)xx * VD_PIL_KMAX] = 1 << 22; }
    a->taps = 1;
  } else {
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    if ((int)std::ceil(support) * 2 + 1 > VD_PIL_KMAX + 8) return 1;   // far past the budget: no table is built
    std::vector<double> wv(VD_PIL_KMAX + 16);
    for (int xx = 0; xx < n_out && fits; ++xx) {
      const double center = (xx + 0.5) * scale;
      int xmin = (int)(center - support + 0.5); if (xmin < 0) xmin = 0;
      int xmax = (int)(center + support + 0.5); if (xmax > n_in) xmax = n_in;
      const int n = xmax - xmin;
      if (n > VD_PIL_KMAX || n < 1) { fits = false; break; }
      double tot = 0.0;
      for (int j = 0; j < n; ++j) { const double v = pr_cubic((j + xmin - center + 0.5) * ss); wv[j] = v; tot += v; }
      const double inv = 1.0 / tot;
      for (int j = 0; j < n; ++j) {
        const double v = tot != 0.0 ? wv[j] * inv : wv[j];
        const int k = v < 0 ? (int)(v * (double)(1 << 22) - 0.5) : (int)(v * (double)(1 << 22) + 0.5);
        if (k >= (1 << 23) || k <= -(1 << 23)) fits = false;   // the 24-bit multiply
        k_v[(size_t)xx * VD_PIL_KMAX + j] = k;
      }
      xmin_v[xx] = xmin; cnt_v[xx] = n;
      if (n > a->taps) a->taps = n;
      if (xx && xmin < xmin_v[xx - 1]) fits = false;   // the kernel takes a tile's first input sample from its first output
    }
    if (!fits) return 1;
  }
  for (int lv = 0; lv < 6; ++lv) {   // the input samples an aligned run of 32 >> lv outputs covers, at most
    const int run = 32 >> lv;
    int span = 0;
    for (int o0 = 0; o0 < n_out; o0 += run) {
      int hi = 0;
      for (int o = o0; o < n_out && o < o0 + run; ++o) hi = std::max(hi, xmin_v[o] + cnt_v[o]);
      span = std::max(span, hi - xmin_v[o0]);
    }
    a->span[lv] = span;
  }
  hipError_t e = hipMalloc((void**)&a->dev, tab.size() * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(a->dev, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice);   // blocking: the table is there before any launch
  if (e != hipSuccess) { if (a->dev) (void)hipFree(a->dev); a->dev = nullptr; *herr = e; return -1; }
  return 0;
}

// float32(float64(v) * (1 / 255)), then (x - mean) / std in float32: DPTImageProcessor's rescale and normalise of the byte v, [3][256] in RGB order
void vd_pil_lut_fill(const float mean[3], const float stdv[3], float* lut768) {
  for (int c = 0; c < 3; ++c)
    for (int v = 0; v < 256; ++v) {
      const float x = (float)((double)v * (1.0 / 255.0));
      lut768[c * 256 + v] = (x - mean[c]) / stdv[c];
    }
}

bool vd_pil_plan(const vd_pil_axis* aw, const vd_pil_axis* ah, int B, int* by_out) {
  if (!aw->dev || !ah->dev || B < 1 || B > 65535) return false;
  if (aw->span[0] * 3 > PR_ROWB) return false;
  int lv = 0;
  while (lv < 6 && ah->span[lv] > PR_HROWS) ++lv;
  if (lv == 6 || (ah->n_out + (32 >> lv) - 1) / (32 >> lv) > 65535) return false;
  *by_out = 32 >> lv;
  return true;
}

// epi 0: uint8 [B][h][w][3] in the input's channel order; VD3D_DT_F32 + 1 / VD3D_DT_BF16 + 1 are not used here: 1 = float32, 2 = bf16 through lut_dev.
// Returns false (nothing launched) where vd_pil_plan refuses the geometry.
bool vd_launch_pil_resample(hipStream_t s, const uint8_t* frames, int B, int H, int W, const vd_pil_axis* aw, const vd_pil_axis* ah, int epi,
                            const float* lut_dev, void* out) {
  int by = 0;
  if (!vd_pil_plan(aw, ah, B, &by) || aw->n_in != W || ah->n_in != H || epi < 0 || epi > 2 || (epi && !lut_dev)) return false;
  const int h = ah->n_out, w = aw->n_out;
  dim3 g((w + PR_SX - 1) / PR_SX, (h + by - 1) / by, B);
  if (epi == 0) hipLaunchKernelGGL(k_pil_resample<0>, g, dim3(256), 0, s, frames, H, W, h, w, aw->dev, ah->dev, by, lut_dev, out);
  else if (epi == 1) hipLaunchKernelGGL(k_pil_resample<1>, g, dim3(256), 0, s, frames, H, W, h, w, aw->dev, ah->dev, by, lut_dev, out);
  else hipLaunchKernelGGL(k_pil_resample<2>, g, dim3(256), 0, s, frames, H, W, h, w, aw->dev, ah->dev, by, lut_dev, out);
  return true;
}
