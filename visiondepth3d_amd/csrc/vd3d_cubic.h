// vd3d_cubic.h -- the two bicubic evaluations more than one kernel file needs, each stated ONCE:
//   rc_*         OpenCV's 8-bit INTER_CUBIC (fixed point: A = -0.75, 11-bit coefficients, one rounding at the end): k_resize_cubic_u8
//                (vd3d_upscale.hip) and the tile gather (vd3d_tiles.hip)
//   bicubic_at   torch's bicubic F.interpolate (align_corners=False) on a float32 plane, in the association of
//                oracle/vd3d_oracle.c:vo_depth_handoff: the depth hand-off (vd3d_handoff.hip) and the tile blend (vd3d_tiles.hip)
#pragma once
#include "vd3d_dev.h"

// ---- OpenCV INTER_CUBIC, 8-bit ------------------------------------------------------------------------------------------
struct rc_axis { int o[4]; int c[4]; };

// coordinate map + coefficients of ONE output index along an axis of source length n (replicate border by index clamping)
VD_DEV rc_axis rc_axis_make(int d, double scale, int n) {
  rc_axis r;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  const float A = -0.75f;
  float w[4];
  w[0] = ((A * (f + 1.f) - 5.f * A) * (f + 1.f) + 8.f * A) * (f + 1.f) - 4.f * A;
  w[1] = ((A + 2.f) * f - (A + 3.f)) * f * f + 1.f;
  w[2] = ((A + 2.f) * (1.f - f) - (A + 3.f)) * (1.f - f) * (1.f - f) + 1.f;
  w[3] = 1.f - w[0] - w[1] - w[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int i = s - 1 + k;
    r.o[k] = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    float v = rintf(w[k] * 2048.f);                       // saturate_cast<short>(cvRound(.))
    r.c[k] = (int)fminf(fmaxf(v, -32768.f), 32767.f);
  }
  return r;
}

// one output pixel (CN interleaved channels) from a source whose rows are `pitch` bytes apart: horizontal pass in int, vertical pass in int,
// (sum + 2^21) >> 22, saturate
template <int CN>
VD_DEV void rc_cubic_pixel(const uint8_t* __restrict__ src, size_t pitch, const rc_axis& ax, const rc_axis& ay, uint8_t* __restrict__ o) {
  int acc[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) acc[c] = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint8_t* row = src + (size_t)ay.o[k] * pitch;
    int h[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) h[c] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint8_t* p = row + (size_t)ax.o[j] * CN;
#pragma unroll
      for (int c = 0; c < CN; ++c) h[c] += (int)p[c] * ax.c[j];
    }
#pragma unroll
    for (int c = 0; c < CN; ++c) acc[c] += h[c] * ay.c[k];
  }
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    const int v = (acc[c] + (1 << 21)) >> 22;
    o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

// ---- torch bicubic (A = -0.75, align_corners=False), float32 -----------------------------------------------------------------
VD_DEV float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
VD_DEV float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
VD_DEV void cubic_coeffs(float t, float c[4]) {
  const float A = -0.75f;
  c[0] = cubic2(t + 1.f, A); c[1] = cubic1(t, A); c[2] = cubic1(1.f - t, A); c[3] = cubic2((1.f - t) + 1.f, A);
}
// value at output column x of the row whose vertical taps are (iy, cy); p: [ph][pw], sw = (float)pw / (float)output width
VD_DEV float bicubic_at(const float* __restrict__ p, int ph, int pw, float sw, const float cy[4], int iy, int x) {
  const float rx = vd_fma(sw, (float)x + 0.5f, -0.5f);   // fused source index, like the bilinear taps (vd3d_dev.h)
  const float fx = floorf(rx);
  const int ix = (int)fx;
  float cx[4];
  cubic_coeffs(rx - fx, cx);
  int xs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { int xx = ix - 1 + j; xs[j] = xx < 0 ? 0 : (xx > pw - 1 ? pw - 1 : xx); }
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int yy = iy - 1 + i; yy = yy < 0 ? 0 : (yy > ph - 1 ? ph - 1 : yy);
    const float* row = p + (size_t)yy * pw;
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) r += row[xs[j]] * cx[j];
    acc += r * cy[i];
  }
  return acc;
}
