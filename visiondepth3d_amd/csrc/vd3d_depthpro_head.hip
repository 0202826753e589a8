// vd3d_depthpro_head.hip -- vd3d_depthpro_head: everything behind head.layers.0 of DepthProDepthEstimationHead as ONE launch on the COARSE map, in both
// arithmetics of the tile convolution (vd3d_conv_x3.h: cx_conv<MODE, CX_T4S2, 8, 1, 3>):
//   ConvTranspose2d(C, C, 2, 2) + bt -> Conv2d(C, 32, 3, padding 1) + b2 -> ReLU -> Conv2d(32, 1, 1) + b3 -> ReLU
// A kernel == stride == 2 transposed convolution followed by a 3 x 3 / padding-1 convolution is, per output phase (p_y, p_x) of the fine grid, a 2 x 2-tap map on
// the coarse grid: phase p reads coarse offsets p - 1 and p -- the tap geometry of CX_T4S2, whose tap (t_y, t_x) of phase (p_y, p_x) is block
// (2 p_y + p_x) * 4 + 2 t_y + t_x of neck_poly_compose(wt, None, w3, 2) (visiondepth3d_amd/depth.py: composed in float64, rounded once).  The biases do not
// compose into one vector: the 3 x 3 convolution pads the FINE map with zeros, not with bt, so the constant term depends on which fine taps fall inside the map --
// the host passes it as a table T[3][3][32] indexed by (first / interior / last fine row, likewise the column).
// Per coarse pixel 16 C x 32 multiply-adds instead of 4 C C + 36 C x 32, and neither 2h x 2w x C map is written.  One fixed summation order (16-channel chunk,
// tap; then the lane butterfly): no split-K, no atomics -- the same bits from call to call and whatever the batch.
// Weight image: [phase 4][chunk C / 16][tap 4] K steps of [term][k-half 2][oc 32][8 bf16 | fp16] (MODE 0: three exact bf16 terms, 3 072 bytes a step; MODE 1: two
// fp16 terms of 2^e W, e per output channel over all 16 blocks as in vd3d_conv_x2t.hip, 2 048 bytes a step, then colscale[32] = 2^-e), then 64 zero bytes.
#include "vd3d_dev.h"
#include "vd3d_conv_x3.h"

static_assert(cx_lds_m(0, 32) <= cx_lds_m(0, 128) && cx_lds_m(1, 32) <= cx_lds_m(1, 128), "inside the tile convolution's LDS plan");

// colscale[oc] = 2^-e over the 16 blocks of Wc [16][32][Cin] (k_conv_x2_scale's rule, vd3d_conv_x2t.hip); one wave per output channel
__global__ __launch_bounds__(256) void k_dph_scale(const float* __restrict__ Wc, int Cin, float* __restrict__ colscale) {
  const int oc = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (oc >= 32) return;
  float mx = 0.f;
  for (int k = lane; k < 16 * Cin; k += 64) mx = fmaxf(mx, fabsf(Wc[((size_t)(k / Cin) * 32 + oc) * Cin + k % Cin]));
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) {
    const int ef = (int)((__float_as_uint(mx) >> 23) & 0xffu);
    int e = 0;
    if (mx > 0.f && ef != 255) { e = 140 - ef; e = e < -100 ? -100 : (e > 100 ? 100 : e); }
    colscale[oc] = __uint_as_float((uint32_t)(127 - e) << 23);
  }
}
// Wc [16][32][Cin] -> the K-step images; one thread = (step, k-half, oc): 8 channels.  step = (phase * nchunk + chunk) * 4 + tap reads block phase * 4 + tap.
template <int MODE>
__global__ __launch_bounds__(256) void k_dph_pack(const float* __restrict__ Wc, int Cin, const float* __restrict__ colscale, uint8_t* __restrict__ img) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int nchunk = Cin / 16, total = 16 * nchunk * 2 * 32;
  if (t >= total) return;
  const int oc = t & 31, khf = (t >> 5) & 1, step = t >> 6;
  const int phase = step / (nchunk * 4), rem = step - phase * (nchunk * 4), c16 = rem >> 2, tap = rem & 3;
  const float* src = Wc + ((size_t)(phase * 4 + tap) * 32 + oc) * Cin + c16 * 16 + khf * 8;
  float w[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) w[e] = src[e];
  uint8_t* base = img + (size_t)step * cx_b_step(MODE, 32) + (khf * 32 + oc) * 16;
  if constexpr (MODE == 0) {
    x3_s8 o[3];
    x3_split8(w, o);
#pragma unroll
    for (int t3 = 0; t3 < 3; ++t3) *reinterpret_cast<uint4*>(base + t3 * 2 * 32 * 16) = __builtin_bit_cast(uint4, o[t3]);
  } else {
    const float sc = 1.0f / colscale[oc];   // a power of two: exact
    x3_h8 h1, h2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = w[e] * sc;
      const _Float16 a1 = (_Float16)v;
      h1[e] = a1; h2[e] = (_Float16)(v - (float)a1);
    }
    *reinterpret_cast<x3_h8*>(base) = h1;
    *reinterpret_cast<x3_h8*>(base + 2 * 32 * 16) = h2;
  }
}

static long long dph_steps_bytes(int mode, int Cin) { return (long long)(Cin / 16) * 16 * cx_b_step(mode, 32); }
long long vd_depthpro_head_weight_bytes(int mode, int Cin) {
  if ((mode != 0 && mode != 1) || Cin < 16 || (Cin & 15) || Cin > 65536) return -1;
  return dph_steps_bytes(mode, Cin) + (mode == 1 ? 32 * 4 : 0) + 64;
}
bool vd_launch_depthpro_head_pack(hipStream_t s, int mode, const float* Wc, int Cin, void* img) {
  const long long wb = vd_depthpro_head_weight_bytes(mode, Cin);
  if (wb < 0 || (reinterpret_cast<uintptr_t>(img) & 15) || (reinterpret_cast<uintptr_t>(Wc) & 3)) return false;
  uint8_t* im = reinterpret_cast<uint8_t*>(img);
  if (hipMemsetAsync(im + wb - 64, 0, 64, s) != hipSuccess) return false;
  const int total = 16 * (Cin / 16) * 2 * 32;
  if (mode == 0) hipLaunchKernelGGL(k_dph_pack<0>, dim3((total + 255) / 256), dim3(256), 0, s, Wc, Cin, (const float*)nullptr, im);
  else {
    float* cs = reinterpret_cast<float*>(im + dph_steps_bytes(1, Cin));
    hipLaunchKernelGGL(k_dph_scale, dim3(8), dim3(256), 0, s, Wc, Cin, cs);
    hipLaunchKernelGGL(k_dph_pack<1>, dim3((total + 255) / 256), dim3(256), 0, s, Wc, Cin, (const float*)cs, im);
  }
  return true;
}

// the entry point has checked every rule; false: the dynamic-LDS attribute could not be set
bool vd_launch_depthpro_head(hipStream_t s, int mode, const float* X, int B, int h, int w, int Cin, const void* wimg, const float* T, const float* w3, float b3,
                             float* out) {
  const long long wb = vd_depthpro_head_weight_bytes(mode, Cin);
  if (wb < 0 || B < 1 || B > 65535 || h < 1 || w < 1) return false;
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_depthpro_head<0>), cx_lds_m(0, 32)}, {reinterpret_cast<const void*>(k_depthpro_head<1>), cx_lds_m(1, 32)}}, attr_set))
    return false;
  const uint8_t* wi = reinterpret_cast<const uint8_t*>(wimg);
  vd_cx_args a;
  a.X = X; a.Wimg = wi; a.zero16 = reinterpret_cast<const float*>(wi + wb - 64); a.bias = T; a.slope = w3; a.R = nullptr; a.Y = out;
  a.B = B; a.H = h; a.W = w; a.Ho = 2 * h; a.Wo = 2 * w;
  a.x_stride = Cin; a.y_stride = 1; a.y_offset = 0; a.r_stride = 0; a.nchunk = Cin / 16;
  a.colscale = mode == 1 ? reinterpret_cast<const float*>(wi + dph_steps_bytes(1, Cin)) : nullptr;
  a.R2 = nullptr; a.Y2 = nullptr; a.relu_in = 0; a.relu = 0; a.b3 = b3;
  a.ntx = (w + CX_TW - 1) / CX_TW;
  const dim3 grid((unsigned)(a.ntx * ((h + CX_TH - 1) / CX_TH)), (unsigned)B, 4u);
  if (mode == 0) hipLaunchKernelGGL(k_depthpro_head<0>, grid, dim3(CX_NT), cx_lds_m(0, 32), s, a);
  else hipLaunchKernelGGL(k_depthpro_head<1>, grid, dim3(CX_NT), cx_lds_m(1, 32), s, a);
  return true;
}
