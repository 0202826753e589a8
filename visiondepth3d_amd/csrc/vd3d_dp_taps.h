// vd3d_dp_taps.h -- ATen's bilinear taps of one axis and the four-tap blend, shared by DepthPro's kernels (vd3d_depthpro.hip, vd3d_depthpro_pyramid.hip).
//
// UpSampleKernel.cpp, align_corners=False, no scale factor given: equal sizes are the identity; otherwise scale = float(in) / out (divided on the host),
// src = max(scale (d + 0.5) - 0.5, 0), i0 = min(floor(src), in - 1), l1 = clamp(src - i0, 0, 1), i1 = i0 + (i0 < in - 1), l0 = 1 - l1, and
// out = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), every operation rounded on its own (-ffp-contract=off).  A zero-weight tap is still multiplied in, as
// ATen does (0 * NaN is NaN in both).
#pragma once
#include "vd3d_dev.h"

struct dp_tap { int i0, i1; float l0, l1; };
VD_DEV dp_tap dp_linear_tap(int d, int in, int out, float scale) {
  dp_tap t;
  if (in == out) { t.i0 = t.i1 = d; t.l0 = 1.f; t.l1 = 0.f; return t; }
  float src = scale * ((float)d + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  int i0 = (int)floorf(src);
  i0 = i0 < in - 1 ? i0 : in - 1;
  float l1 = src - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
  t.i0 = i0; t.i1 = i0 + (i0 < in - 1 ? 1 : 0); t.l1 = l1; t.l0 = 1.f - l1;
  return t;
}
VD_DEV float dp_blend(const dp_tap& ty, const dp_tap& tx, float v00, float v01, float v10, float v11) {
  const float top = tx.l0 * v00 + tx.l1 * v01, bot = tx.l0 * v10 + tx.l1 * v11;
  return ty.l0 * top + ty.l1 * bot;
}
