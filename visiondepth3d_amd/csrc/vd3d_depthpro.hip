// vd3d_depthpro.hip -- the two memory-bound kernels around DepthPro (DepthProForDepthEstimation) in DepthPipe: the image processor's front end and the
// field-of-view / inverse-depth post-process.  visiondepth3d_amd/depth_pro.py states both in torch; tests/test_hip_depth_pro_kernels.py holds the kernels to them.
//
// k_dp_preprocess: uint8 BGR [B][H][W][3] -> float32 planar [B][3][S][S].  The processor rescales and normalises FIRST ((byte - 255 mean) / (255 std): a table of
//                  the byte, 3 x 256 floats in LDS, built per workgroup) and resizes the float image afterwards, bilinear without antialias.  One thread = 4
//                  neighbouring output pixels of all three planes: three 16-byte stores, every source byte read once per thread.  The table was measured
//                  against computing the subtraction and the division at every tap (48 correctly rounded divisions per thread, no LDS, no barrier; the same
//                  bits): 0.088 ms against 0.114 ms for eight 1080p frames, 0.0166 against 0.0202 for one (profiles/r25_depth_pro.md) -- the table stays.
// k_dp_post:       prediction [B][S][S] (+ field of view [B] in degrees, read on the device) -> [B][oH][oW]: depth * width / focal, focal = 0.5 width /
//                  tan(0.5 deg2rad(fov)) (tan evaluated in float64 and narrowed: within 1 ulp of float32), bilinear resize, clamp to [1e-4, 1e4] (NaN stays NaN),
//                  reciprocal.
//
// The bilinear taps (vd3d_dp_taps.h) are ATen's (UpSampleKernel.cpp, align_corners=False, no scale factor given): equal sizes are the identity; otherwise scale = float(in) / out
// (divided on the host), src = max(scale (d + 0.5) - 0.5, 0), i0 = min(floor(src), in - 1), l1 = clamp(src - i0, 0, 1), i1 = i0 + (i0 < in - 1), l0 = 1 - l1, and
// out = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), every operation rounded on its own (-ffp-contract=off).  A zero-weight tap is still multiplied in, as
// ATen does (0 * NaN is NaN in both).
#include "vd3d_dev.h"
#include "vd3d_dp_taps.h"
#include "vd3d_kernels.h"

struct dp_norm { float m[3], s[3]; };   // 255 mean, 255 std in R, G, B order

__global__ __launch_bounds__(256) void k_dp_preprocess(const uint8_t* __restrict__ frames, int H, int W, int S, float sy, float sx, dp_norm nm, long long total,
                                                       float* __restrict__ out) {
  __shared__ float tab[3 * 256];   // three divisions per thread, once per workgroup, instead of 48: the correctly rounded division is a dozen instructions
  for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = ((float)(i & 255) - nm.m[i >> 8]) / nm.s[i >> 8];
  __syncthreads();
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int s4 = S >> 2;
  const int x4 = (int)(idx % s4);
  long long r = idx / s4;
  const int y = (int)(r % S);
  const long long b = r / S;
  const dp_tap ty = dp_linear_tap(y, H, S, sy);
  const uint8_t* r0 = frames + (b * H + ty.i0) * (long long)W * 3;
  const uint8_t* r1 = frames + (b * H + ty.i1) * (long long)W * 3;
  float o[3][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const dp_tap tx = dp_linear_tap(x4 * 4 + e, W, S, sx);
    const int a = tx.i0 * 3, c = tx.i1 * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {   // plane ch (R, G, B) reads byte 2 - ch of the BGR pixel
      const float* t = tab + ch * 256;
      o[ch][e] = dp_blend(ty, tx, t[r0[a + 2 - ch]], t[r0[c + 2 - ch]], t[r1[a + 2 - ch]], t[r1[c + 2 - ch]]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    *reinterpret_cast<float4*>(out + ((b * 3 + ch) * S + y) * (long long)S + x4 * 4) = float4{o[ch][0], o[ch][1], o[ch][2], o[ch][3]};
}

// false = nothing launched (the caller has checked the shapes): a grid past 2^31 - 1 workgroups
bool vd_launch_depthpro_preprocess_u8(hipStream_t s, const uint8_t* frames, int B, int H, int W, int S, const float mean[3], const float std[3], float* out) {
  const long long total = (long long)B * S * (S / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  dp_norm nm;
  const float k = (float)(1.0 / (1.0 / 255));   // the processor's 1 / rescale_factor, narrowed as the float32 tensor product narrows it
  for (int c = 0; c < 3; ++c) { nm.m[c] = mean[c] * k; nm.s[c] = std[c] * k; }
  hipLaunchKernelGGL(k_dp_preprocess, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, H, W, S, (float)H / (float)S, (float)W / (float)S, nm, total, out);
  return true;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_dp_post(const float* __restrict__ pred, const float* __restrict__ fov, int S, int oH, int oW, float sy, float sx, int resize,
                                                 long long per, long long total, float* __restrict__ out) {
  const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  const float width = (float)oW, half_width = 0.5f * (float)oW;
  long long cur = -1;
  float focal = 1.f;
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long el = e0 + e;
    o[e] = 0.f;
    if (el >= total) continue;
    const long long b = el / per, rem = el - b * per;
    const int y = (int)(rem / oW), x = (int)(rem - (long long)y * oW);
    if (fov && b != cur) {   // focal = 0.5 width / tan(0.5 deg2rad(fov)); deg2rad multiplies by float32(pi / 180)
      const float hf = 0.5f * (fov[b] * 0.017453292519943295f);
      focal = half_width / (float)tan((double)hf);
      cur = b;
    }
    const float* pb = pred + b * (long long)S * S;
    float v;
    if (!resize) {
      v = pb[(long long)y * S + x];
      if (fov) v = (v * width) / focal;
    } else {
      const dp_tap ty = dp_linear_tap(y, S, oH, sy), tx = dp_linear_tap(x, S, oW, sx);
      float v00 = pb[(long long)ty.i0 * S + tx.i0], v01 = pb[(long long)ty.i0 * S + tx.i1], v10 = pb[(long long)ty.i1 * S + tx.i0], v11 = pb[(long long)ty.i1 * S + tx.i1];
      if (fov) { v00 = (v00 * width) / focal; v01 = (v01 * width) / focal; v10 = (v10 * width) / focal; v11 = (v11 * width) / focal; }
      v = dp_blend(ty, tx, v00, v01, v10, v11);
    }
    o[e] = 1.0f / vd_clamp(v, 1e-4f, 1e4f);   // NaN passes both comparisons and stays NaN
  }
  if (VEC && e0 + 3 < total) { *reinterpret_cast<float4*>(out + e0) = float4{o[0], o[1], o[2], o[3]}; return; }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e0 + e < total) out[e0 + e] = o[e];
}

// The caller has checked the shapes.  16-byte stores where out is 16-byte aligned (the output is walked as one flat array), 4-byte stores otherwise.  false: a grid too large.
bool vd_launch_depthpro_post_f32(hipStream_t s, const float* pred, const float* fov, int B, int S, int oH, int oW, float* out) {
  const long long per = (long long)oH * oW, total = per * B, threads = (total + 3) / 4;
  if ((threads + 255) / 256 > 0x7fffffffLL) return false;
  const int resize = !(oH == S && oW == S);
  const dim3 g((unsigned)((threads + 255) / 256)), blk(256);
  const float sy = (float)S / (float)oH, sx = (float)S / (float)oW;
  if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) hipLaunchKernelGGL(k_dp_post<true>, g, blk, 0, s, pred, fov, S, oH, oW, sy, sx, resize, per, total, out);
  else hipLaunchKernelGGL(k_dp_post<false>, g, blk, 0, s, pred, fov, S, oH, oW, sy, sx, resize, per, total, out);
  return true;
}
