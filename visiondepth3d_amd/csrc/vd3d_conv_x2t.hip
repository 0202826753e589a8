// vd3d_conv_x2t.hip -- vd3d_conv3x3_s1_x2 and vd3d_conv3x3_s2_x2: the tile convolution of vd3d_conv_x3.h (8 x 32 output tile, halo tile staged once per
// 16-channel chunk, weight ring of four stages, C_out slices on the grid's z axis; the plan: vd3d_conv_x3.hip's header comment) in the fp16x2 arithmetic of
// vd3d_x3.h MODE 1, for the 3 x 3 convolutions of the DPT neck / fusion stage / head (stride 1, C_out 32 / 64 / 128 / 256) and of the reassemble stage (stride 2,
// C_out = 128 n).  Float32 NHWC in and out, dense maps, no bias.
// Arithmetic: x ~ h1 + h2 with h1 = fp16(x), h2 = fp16(x - h1), round to nearest, split in the kernel; weights as 2^e W ~ g1 + g2 the same way, split by the
// packer, with e per output channel such that max |2^e W| lies in [2^13, 2^14) (second terms stay normal fp16 numbers down to 2^-24 of the channel's largest
// weight).  h1 g1 goes into `acc`, h1 g2 and h2 g1 into `lo` (v_mfma_f32_32x32x16_f16, float32 accumulation), h2 g2 <= 2^-22 relative is dropped; the epilogue
// stores (acc + lo) * 2^-e -- a power of two, exact.  |x| must stay below 65 504: a larger x splits into Inf - Inf and every output whose window holds it is
// non-finite, never a finite wrong number.
// Weight image: [slice][step][term 2][k-half 2][oc CK][8 fp16] (64 CK bytes per step, CK = min(C_out, 128), the steps of a slice contiguous and in the order a
// workgroup runs them: vd3d_conv_x3.hip), then colscale[C_out] = 2^-e as float32, then 64 zero bytes (the zero page of the padding and of DMA lanes past a step).
// c2t_launch selects the kernel; the checks, the argument block and the grid are cx_dense_args's (vd3d_conv_x3.h).
#include "vd3d_dev.h"
#include "vd3d_conv_x3.h"

static_assert(cx_lds_m(1, 32) == 100864 && cx_lds_m(1, 64) == 100864 && cx_lds_m(1, 128) == 100864 && cx_b_stage_m(1, 128) == CX_NT * 16, "LDS plan: one DMA round per B stage");

// ---- colscale[oc] = 2^-e, e = 13 - floor(log2 max |W[oc]|) read from the exponent field (exact), clamped to +-100; an all-zero or non-finite channel: e = 0
__global__ __launch_bounds__(256) void k_conv_x2_scale(const float* __restrict__ W, int Cout, int per_oc, float* __restrict__ colscale) {
  const int oc = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (oc >= Cout) return;
  float mx = 0.f;
  for (int k = lane; k < per_oc; k += 64) mx = fmaxf(mx, fabsf(W[(size_t)oc * per_oc + k]));
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) {
    const int ef = (int)((__float_as_uint(mx) >> 23) & 0xffu);
    int e = 0;
    if (mx > 0.f && ef != 255) { e = 140 - ef; e = e < -100 ? -100 : (e > 100 ? 100 : e); }   // a subnormal maximum: ef = 0, clamped
    colscale[oc] = __uint_as_float((uint32_t)(127 - e) << 23);
  }
}
// ---- weights W[Cout][Cin][3][3] -> the K-step images; one thread = (step, k-half, oc): 8 channels.  The step order is k_conv_x3_pack's (vd3d_conv_x3.hip).
__global__ __launch_bounds__(256) void k_conv_x2_pack(int kind, const float* __restrict__ W, int Cout, int Cin, const float* __restrict__ colscale, uint8_t* __restrict__ img) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int nchunk = Cin / 16, total = nchunk * 9 * 2 * Cout;
  if (t >= total) return;
  const int oc = t % Cout, khf = (t / Cout) & 1, CK = Cout > 128 ? 128 : Cout;
  int step = t / (2 * Cout), ky, kx;
  const int c16 = step / 9, j = step - c16 * 9;
  if (kind == CX_K3S1) { ky = j / 3; kx = j - ky * 3; }
  else {   // per 16 channels: sub-pixel (0,0) 1 step, (0,1) 2, (1,0) 2, (1,1) 4
    const int sub = j == 0 ? 0 : j < 3 ? 1 : j < 5 ? 2 : 3, tap = j == 0 ? 0 : j < 3 ? j - 1 : j < 5 ? j - 3 : j - 5;
    const int sy = sub >> 1, sx = sub & 1, ty = sx ? tap >> 1 : tap, tx = sx ? tap & 1 : 0;
    ky = sy ? 2 * ty : 1; kx = sx ? 2 * tx : 1;
  }
  step += (oc / CK) * nchunk * 9;
  const float sc = 1.0f / colscale[oc];   // a power of two: exact
  x3_h8 h1, h2;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ci = c16 * 16 + khf * 8 + e;
    const float v = W[(((size_t)oc * Cin + ci) * 3 + ky) * 3 + kx] * sc;
    const _Float16 a1 = (_Float16)v;
    h1[e] = a1; h2[e] = (_Float16)(v - (float)a1);
  }
  uint8_t* base = img + (size_t)step * CK * 64 + (khf * CK + oc % CK) * 16;
  *reinterpret_cast<x3_h8*>(base) = h1;
  *reinterpret_cast<x3_h8*>(base + 2 * CK * 16) = h2;
}

static bool c2t_cin_ok(int Cin) { return Cin >= 16 && (Cin & 15) == 0 && Cin <= 65536; }
static long long c2t_steps_bytes(int Cin, int Cout) { return (long long)(Cin / 16) * 9 * Cout * 64; }
long long vd_conv3x3_s1_x2_weight_bytes(int Cin, int Cout) {
  if (!c2t_cin_ok(Cin) || (Cout != 32 && Cout != 64 && Cout != 128 && Cout != 256)) return -1;
  return c2t_steps_bytes(Cin, Cout) + (long long)Cout * 4 + 64;
}
long long vd_conv3x3_s2_x2_weight_bytes(int Cin, int Cout) {
  if (!c2t_cin_ok(Cin) || Cout < 128 || (Cout & 127) || Cout > 1024) return -1;
  return c2t_steps_bytes(Cin, Cout) + (long long)Cout * 4 + 64;
}
static bool c2t_pack(hipStream_t s, int kind, const float* W, int Cin, int Cout, void* img) {
  if (reinterpret_cast<uintptr_t>(img) & 15) return false;
  uint8_t* im = reinterpret_cast<uint8_t*>(img);
  const long long sb = c2t_steps_bytes(Cin, Cout);
  float* cs = reinterpret_cast<float*>(im + sb);
  if (hipMemsetAsync(im + sb + (long long)Cout * 4, 0, 64, s) != hipSuccess) return false;
  hipLaunchKernelGGL(k_conv_x2_scale, dim3((Cout + 3) / 4), dim3(256), 0, s, W, Cout, Cin * 9, cs);
  const int total = (Cin / 16) * 9 * 2 * Cout;
  hipLaunchKernelGGL(k_conv_x2_pack, dim3((total + 255) / 256), dim3(256), 0, s, kind, W, Cout, Cin, (const float*)cs, im);
  return true;
}
bool vd_launch_conv3x3_s1_x2_pack(hipStream_t s, const float* W, int Cin, int Cout, void* img) {
  return vd_conv3x3_s1_x2_weight_bytes(Cin, Cout) >= 0 && c2t_pack(s, CX_K3S1, W, Cin, Cout, img);
}
bool vd_launch_conv3x3_s2_x2_pack(hipStream_t s, const float* W, int Cin, int Cout, void* img) {
  return vd_conv3x3_s2_x2_weight_bytes(Cin, Cout) >= 0 && c2t_pack(s, CX_K3S2, W, Cin, Cout, img);
}

// the entry points have checked the shape; false: a broken pointer rule, or the dynamic-LDS attribute could not be set
static bool c2t_launch(hipStream_t s, int kind, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, float* Y) {
  const float* cs = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(wimg) + c2t_steps_bytes(Cin, Cout));   // colscale[C_out], then the zero page
  vd_cx_args a;
  dim3 grid;
  if (!cx_dense_args(kind, X, B, H, W, Cin, wimg, Cout, Y, cs, cs + Cout, a, grid)) return false;
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_conv_x2<CX_K3S1, 8, 1>), cx_lds_m(1, 32)}, {reinterpret_cast<const void*>(k_conv_x2<CX_K3S1, 4, 1>), cx_lds_m(1, 64)},
                     {reinterpret_cast<const void*>(k_conv_x2<CX_K3S1, 4, 2>), cx_lds_m(1, 128)}, {reinterpret_cast<const void*>(k_conv_x2<CX_K3S2, 4, 2>), cx_lds_m(1, 128)}},
                    attr_set)) return false;
  if (kind == CX_K3S2) hipLaunchKernelGGL((k_conv_x2<CX_K3S2, 4, 2>), grid, dim3(CX_NT), cx_lds_m(1, 128), s, a);
  else if (Cout == 32) hipLaunchKernelGGL((k_conv_x2<CX_K3S1, 8, 1>), grid, dim3(CX_NT), cx_lds_m(1, 32), s, a);   // the head's 64 -> 32
  else if (Cout == 64) hipLaunchKernelGGL((k_conv_x2<CX_K3S1, 4, 1>), grid, dim3(CX_NT), cx_lds_m(1, 64), s, a);
  else hipLaunchKernelGGL((k_conv_x2<CX_K3S1, 4, 2>), grid, dim3(CX_NT), cx_lds_m(1, 128), s, a);   // 128, or 256 as two slices
  return true;
}
bool vd_launch_conv3x3_s1_x2(hipStream_t s, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, float* Y) {
  return vd_conv3x3_s1_x2_weight_bytes(Cin, Cout) >= 0 && c2t_launch(s, CX_K3S1, X, B, H, W, Cin, wimg, Cout, Y);
}
bool vd_launch_conv3x3_s2_x2(hipStream_t s, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, float* Y) {
  return vd_conv3x3_s2_x2_weight_bytes(Cin, Cout) >= 0 && c2t_launch(s, CX_K3S2, X, B, H, W, Cin, wimg, Cout, Y);
}
