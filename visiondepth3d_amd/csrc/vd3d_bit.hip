// vd3d_bit.hip -- the memory-bound kernels of the BiT ResNet prefix of DPT-Hybrid (MiDaS 3.0) under DepthPipe(self_contained=True): the matrix work runs on
// vd3d_gemm_x3 and the tile convolutions; these three kernels are the rest.  Activations are float32 NHWC rows [B * H * W][C] throughout.
//
// k_im2col:   the gather of k x k windows (k = 1 | 3 | 7, stride 1 | 2, zero padding given per side) into GEMM rows [B * Ho * Wo][Kp], column (ky * k + kx) * C + c,
//             Kp = k k C rounded up to 16 with a zero tail.  Exact copies; one thread = 4 columns (one 16-byte store; one 16-byte load where C % 4 == 0).
// k_maxpool:  3 x 3 / stride 2 max-pool with padding per side and a pad value, torch's update rule (v > m or v is NaN).  One thread = 4 channels of one output pixel.
// GroupNorm:  out = [relu]((x - mean_g) * rstd_g * gamma[c] + beta[c] [+ residual]) per (frame, group), biased variance, in three launches
//             (k_gn_stats<0>: partial sums; k_gn_stats<1>: partial centred sums of squares; k_gn_apply), because the mean has to be complete before the second pass
//             starts and nothing here waits across workgroups.  No atomics; ONE summation order, a function of (P, C, C / G) alone -- not of the batch, the grid or
//             the device (tests/test_hip_bit_stem.py states it in NumPy):
//               1. a frame's P pixels are cut into chunks of CH = max(16, ceil(P / 64) rounded up to 16) pixels: at most 64 chunks, one workgroup each;
//               2. in a chunk, with R = 1024 / C pixel rows in flight, row r sums the pixels r, r + R, r + 2R, ... of the chunk one after the other, per channel,
//                  starting from 0 (second pass: the squares (x - mean_g)^2, multiply and add rounded separately);
//               3. the C / G channel sums of a group are added as a pairwise tree of neighbours (v[0] + v[1], v[2] + v[3], ... until one is left);
//               4. the R rows, padded with zeros to 16, are added as the same pairwise tree;
//               5. the chunks' partials, padded with zeros to 64, are added as the same pairwise tree (every consumer workgroup redoes it: one wave per group);
//               6. mean = sum / (P C / G), a float32 division; rstd = 1 / sqrt(centred sum / (P C / G) + eps) in float64 from the float32 sum (division, square
//                  root and reciprocal each correctly rounded), and the channel's scale s_c = float32(rstd * gamma[c]): one rounding to float32 where a float32
//                  chain has four (the statistics' error multiplies every value of the group).
//             The apply pass computes (x - mean) * s_c + beta, then + residual, then y < 0 ? 0 : y: every operation rounded on its own (-ffp-contract=off).
#include "vd3d_dev.h"
#include "vd3d_kernels.h"

template <bool VEC>
__global__ __launch_bounds__(256) void k_im2col(const float* __restrict__ x, int H, int W, int C, int k, int stride, int pt, int pl, int Ho, int Wo, int kp4,
                                                long long total, float4* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k4 = (int)(idx % kp4);
  long long r = idx / kp4;
  const int ox = (int)(r % Wo); r /= Wo;
  const int oy = (int)(r % Ho);
  const long long b = r / Ho;
  const int K = k * k * C;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {   // C % 4 == 0: the four columns lie in one tap
    const int col = k4 * 4;
    if (col < K) {
      const int tap = col / C, c = col - tap * C, ky = tap / k, kx = tap - ky * k;
      const int iy = oy * stride - pt + ky, ix = ox * stride - pl + kx;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const float4 t = *reinterpret_cast<const float4*>(x + ((b * H + iy) * W + ix) * C + c);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = k4 * 4 + e;
      if (col < K) {
        const int tap = col / C, c = col - tap * C, ky = tap / k, kx = tap - ky * k;
        const int iy = oy * stride - pt + ky, ix = ox * stride - pl + kx;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v[e] = x[((b * H + iy) * W + ix) * C + c];
      }
    }
  }
  out[idx] = float4{v[0], v[1], v[2], v[3]};
}

// false = nothing launched: k not 1 / 3 / 7, stride not 1 / 2, a padding outside 0 .. k - 1, no output pixel, a grid past 2^31 - 1 workgroups, rows not 16-byte
// aligned or x not 4-byte (16-byte where C % 4 == 0: the vector form).
bool vd_launch_im2col_nhwc_f32(hipStream_t s, const float* x, int B, int H, int W, int C, int k, int stride, int pt, int pb, int pl, int pr, float* rows) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || (k != 1 && k != 3 && k != 7) || (stride != 1 && stride != 2)) return false;
  if (pt < 0 || pb < 0 || pl < 0 || pr < 0 || pt >= k || pb >= k || pl >= k || pr >= k) return false;
  if (H + pt + pb < k || W + pl + pr < k) return false;
  const int Ho = (H + pt + pb - k) / stride + 1, Wo = (W + pl + pr - k) / stride + 1;
  const long long K = (long long)k * k * C;
  if (K > (1 << 20)) return false;
  const int kp = (int)((K + 15) / 16 * 16);
  const bool vec = C % 4 == 0;
  if ((reinterpret_cast<uintptr_t>(x) & (vec ? 15 : 3)) || (reinterpret_cast<uintptr_t>(rows) & 15)) return false;
  const long long total = (long long)B * Ho * Wo * (kp / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  const dim3 g((unsigned)((total + 255) / 256)), blk(256);
  if (vec) hipLaunchKernelGGL(k_im2col<true>, g, blk, 0, s, x, H, W, C, k, stride, pt, pl, Ho, Wo, kp / 4, total, (float4*)rows);
  else hipLaunchKernelGGL(k_im2col<false>, g, blk, 0, s, x, H, W, C, k, stride, pt, pl, Ho, Wo, kp / 4, total, (float4*)rows);
  return true;
}

__global__ __launch_bounds__(256) void k_maxpool3x3_s2(const float4* __restrict__ x, int H, int W, int c4, int pt, int pl, float pad, int Ho, int Wo, long long total,
                                                       float4* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % c4);
  long long r = idx / c4;
  const int ox = (int)(r % Wo); r /= Wo;
  const int oy = (int)(r % Ho);
  const long long b = r / Ho;
  const float ninf = -__builtin_huge_valf();
  float4 m = float4{ninf, ninf, ninf, ninf};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = oy * 2 - pt + ky, ix = ox * 2 - pl + kx;
      float4 v = float4{pad, pad, pad, pad};
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[((b * H + iy) * W + ix) * c4 + c];
      m.x = (v.x > m.x || v.x != v.x) ? v.x : m.x;   // torch's max_pool2d: a NaN in the window is the result
      m.y = (v.y > m.y || v.y != v.y) ? v.y : m.y;
      m.z = (v.z > m.z || v.z != v.z) ? v.z : m.z;
      m.w = (v.w > m.w || v.w != v.w) ? v.w : m.w;
    }
  }
  out[idx] = m;
}

// false = nothing launched: C not a multiple of 4, a padding outside 0 .. 2, no output pixel, a grid past 2^31 - 1 workgroups, x / out not 16-byte aligned.
bool vd_launch_maxpool3x3_s2_nhwc_f32(hipStream_t s, const float* x, int B, int H, int W, int C, int pt, int pb, int pl, int pr, float pad, float* out) {
  if (B < 1 || H < 1 || W < 1 || C < 4 || C % 4 || pt < 0 || pb < 0 || pl < 0 || pr < 0 || pt > 2 || pb > 2 || pl > 2 || pr > 2) return false;
  if (H + pt + pb < 3 || W + pl + pr < 3) return false;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) return false;
  const int Ho = (H + pt + pb - 3) / 2 + 1, Wo = (W + pl + pr - 3) / 2 + 1;
  const long long total = (long long)B * Ho * Wo * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  hipLaunchKernelGGL(k_maxpool3x3_s2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float4*)x, H, W, C / 4, pt, pl, pad, Ho, Wo, total, (float4*)out);
  return true;
}

// ---- GroupNorm
// the chunk length of step 1 (host and device agree through this one function)
static inline int gn_chunk(long long P) {
  long long ch = ((P + 63) / 64 + 15) / 16 * 16;
  return (int)(ch < 16 ? 16 : ch);
}
static inline bool gn_shape_ok(int B, long long P, int C, int G) {
  if (B < 1 || B > 65535 || P < 1 || P > (1LL << 24) || G < 1 || C < 1 || C % G) return false;
  const int cpg = C / G;
  return (C == 64 || C == 128 || C == 256 || C == 512 || C == 1024) && (cpg == 2 || cpg == 4 || cpg == 8 || cpg == 16 || cpg == 32);
}
// < 0: shape not built.  Per frame and chunk slot (64 of them) one float per group, for the sums and for the centred sums of squares.
long long vd_groupnorm_workspace_bytes(int B, long long P, int C, int G) {
  return gn_shape_ok(B, P, C, G) ? (long long)B * 2 * 64 * G * (long long)sizeof(float) : -1;
}

// step 5: the pairwise tree over the 64 chunk slots of group g (part: [G][64]; chunk 0's workgroup has written zeros to the slots no chunk owns), one wave per
// group and one slot per lane: the xor butterfly 1, 2, 4, ... 32 leaves v[0::2] + v[1::2], repeated, in every lane (a + b and b + a are the same float).
VD_DEV float gn_tree64(const float* __restrict__ part, int g, int lane) {
  float v = part[(long long)g * 64 + lane];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// PASS 0: partial sums; PASS 1: partial centred sums of squares (reads pass 0's partials for the mean).  grid (chunks, B), 256 threads = R pixel rows x C / 4 columns.
template <int PASS>
__global__ __launch_bounds__(256) void k_gn_stats(const float4* __restrict__ x, int P, int C, int cpg, int ch, float* __restrict__ ws) {
  __shared__ float s_mean[512];
  __shared__ float s_row[512];
  const int t = threadIdx.x, c4 = C >> 2, G = C / cpg, R = 256 / c4;
  const int nch = (P + ch - 1) / ch, chunk = blockIdx.x, b = blockIdx.y;
  float* sums = ws + (long long)b * 2 * 64 * G;   // [G][64] sums, then [G][64] centred squares
  const int row = t / c4, col = t - row * c4;
  float m[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (PASS == 1) {
    const float n = (float)((long long)P * cpg);
    for (int g = t >> 6; g < G; g += 4) {
      const float v = gn_tree64(sums, g, t & 63);
      if ((t & 63) == 0) s_mean[g] = v / n;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = s_mean[(col * 4 + e) / cpg];
  }
  const int p0 = chunk * ch, n_c = min(ch, P - p0);
  const float4* xp = x + ((long long)b * P + p0) * c4 + col;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (int p = row; p < n_c; p += R) {
    const float4 v = xp[(long long)p * c4];
    if constexpr (PASS == 0) {
      a[0] = a[0] + v.x; a[1] = a[1] + v.y; a[2] = a[2] + v.z; a[3] = a[3] + v.w;
    } else {
      const float d0 = v.x - m[0], d1 = v.y - m[1], d2 = v.z - m[2], d3 = v.w - m[3];
      a[0] = a[0] + d0 * d0; a[1] = a[1] + d1 * d1; a[2] = a[2] + d2 * d2; a[3] = a[3] + d3 * d3;
    }
  }
  // step 3: the channels of a group as a pairwise tree -- in the thread, then across the cpg / 4 neighbouring lanes (aligned: c4 is a multiple of cpg / 4)
  const float lo = a[0] + a[1], hi = a[2] + a[3];
  if (cpg == 2) {
    s_row[row * G + col * 2] = lo;
    s_row[row * G + col * 2 + 1] = hi;
  } else {
    float v = lo + hi;
    for (int off = 1; off < (cpg >> 2); off <<= 1) v = v + __shfl_xor(v, off, 64);
    if ((col & ((cpg >> 2) - 1)) == 0) s_row[row * G + col / (cpg >> 2)] = v;
  }
  __syncthreads();
  // step 4: the R rows (a power of two up to 16) as a pairwise tree, one thread per group
  float* dst = sums + (PASS ? 64 * G : 0) + chunk;
  for (int g = t; g < G; g += 256) {
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = r < R ? s_row[r * G + g] : 0.f;
#pragma unroll
    for (int n = 16; n > 1; n >>= 1) {
#pragma unroll
      for (int i = 0; i < n / 2; ++i) v[i] = v[2 * i] + v[2 * i + 1];
    }
    // (rows from R on are zeros: adding them leaves the tree of the first R rows, bit for bit, for a power of two R)
    dst[g * 64] = v[0];
    if (chunk == 0)   // the slots behind the last chunk: zeros for step 5
      for (int j = nch; j < 64; ++j) dst[g * 64 + j] = 0.f;
  }
}

// flags: 1 = ReLU.  x, res and out may be the same array (each thread reads an element before it writes it).
__global__ __launch_bounds__(256) void k_gn_apply(const float4* x, const float4* res, const float4* __restrict__ gamma, const float4* __restrict__ beta, float eps, int relu,
                                                  int P, int C, int cpg, int ch, const float* __restrict__ ws, float4* out) {
  __shared__ float s_mean[512];
  __shared__ double s_rstd[512];
  const int t = threadIdx.x, c4 = C >> 2, G = C / cpg, R = 256 / c4;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const float* sums = ws + (long long)b * 2 * 64 * G;
  const float n = (float)((long long)P * cpg);
  for (int g = t >> 6; g < G; g += 4) {
    const float sm = gn_tree64(sums, g, t & 63), sq = gn_tree64(sums + 64 * G, g, t & 63);
    if ((t & 63) == 0) {
      s_mean[g] = sm / n;
      s_rstd[g] = 1.0 / sqrt((double)sq / (double)n + (double)eps);
    }
  }
  __syncthreads();
  const int row = t / c4, col = t - row * c4;
  const float4 ga = gamma[col], be = beta[col];
  const float gam[4] = {ga.x, ga.y, ga.z, ga.w};
  float m[4], sc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { m[e] = s_mean[(col * 4 + e) / cpg]; sc[e] = (float)(s_rstd[(col * 4 + e) / cpg] * (double)gam[e]); }
  const int p0 = chunk * ch, n_c = min(ch, P - p0);
  const long long base = ((long long)b * P + p0) * c4 + col;
  for (int p = row; p < n_c; p += R) {
    const long long i = base + (long long)p * c4;
    const float4 v = x[i];
    float4 y;
    y.x = (v.x - m[0]) * sc[0] + be.x;
    y.y = (v.y - m[1]) * sc[1] + be.y;
    y.z = (v.z - m[2]) * sc[2] + be.z;
    y.w = (v.w - m[3]) * sc[3] + be.w;
    if (res) { const float4 q = res[i]; y.x = y.x + q.x; y.y = y.y + q.y; y.z = y.z + q.z; y.w = y.w + q.w; }
    if (relu) { y.x = y.x < 0.f ? 0.f : y.x; y.y = y.y < 0.f ? 0.f : y.y; y.z = y.z < 0.f ? 0.f : y.z; y.w = y.w < 0.f ? 0.f : y.w; }   // a NaN stays a NaN
    out[i] = y;
  }
}

// false = nothing launched: a shape vd_groupnorm_workspace_bytes refuses, or x / res / gamma / beta / ws / out not 16-byte aligned.
bool vd_launch_groupnorm_nhwc_f32(hipStream_t s, const float* x, const float* res, const float* gamma, const float* beta, float eps, int relu, int B, long long P, int C,
                                  int G, void* ws, float* out) {
  if (!gn_shape_ok(B, P, C, G)) return false;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) |
       reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(out)) & 15) return false;
  const int ch = gn_chunk(P), nch = (int)((P + ch - 1) / ch), cpg = C / G;
  const dim3 g((unsigned)nch, (unsigned)B), blk(256);
  hipLaunchKernelGGL(k_gn_stats<0>, g, blk, 0, s, (const float4*)x, (int)P, C, cpg, ch, (float*)ws);
  hipLaunchKernelGGL(k_gn_stats<1>, g, blk, 0, s, (const float4*)x, (int)P, C, cpg, ch, (float*)ws);
  hipLaunchKernelGGL(k_gn_apply, g, blk, 0, s, (const float4*)x, (const float4*)res, (const float4*)gamma, (const float4*)beta, eps, relu, (int)P, C, cpg, ch,
                     (const float*)ws, (float4*)out);
  return true;
}
