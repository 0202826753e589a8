// vd3d_depthpro_pyramid.hip -- the two memory-bound gathers around DepthPro's three ViT encoders under DepthPipe(encoders=...): the patch pyramid in front of the
// patch encoder and the patch merge behind every encoder.  visiondepth3d_amd/depth_pro.py states both in NumPy (patches_statement, merge_statement);
// tests/test_hip_depth_pro_pyramid.py holds the kernels to them bit for bit.  No LDS, no atomics, 256-thread workgroups.
//
// k_dp_patches: float32 planar pixel_values [B][3][S][S] (S a multiple of 4) -> the whole stack DepthProPatchEncoder hands its ViT, [(n1^2 + n2^2 + n4^2) B]
//               patches of p x p: the full-resolution level first, then the half, then the quarter; inside a level patch-major, batch-minor (index l B + b).  The
//               two scaled levels are 0.25 ((a + b) + (c + d)) over the 2 x 2 cell (half) and over the 2 x 2 centre of the 4 x 4 cell (quarter): F.interpolate(
//               scale_factor=0.5 / 0.25, bilinear) on such sides, every weight exactly 0.5.  One launch instead of two interpolations, the slices and a
//               concatenation.  The patches are written pixel-interleaved, [N][p][p][3] -- the channels_last memory vd3d_patchify_f32 reads.
//               <true>:  one thread = 4 neighbouring pixels of all three channels: 16-byte loads, three 16-byte stores (48 contiguous bytes).  Needs p and every
//                        stride in use a multiple of 4.
//               <false>: one thread = one pixel, 4-byte loads and stores: any p and stride (strides of 15 / 10 for p = 20).
// k_dp_merge:   token rows [n B][T][C] (a level's slice of an encoder output or of a hook's hidden state) -> reconstruct_feature_maps in NHWC, [B][oh][ow][C]: the
//               leading T - g^2 tokens dropped, side = int(sqrt(n)) patches per side (sequences past side^2 are never read), pad tokens trimmed on the edges
//               that meet another patch, then ATen's bilinear taps (vd3d_dp_taps.h) -- skipped where the merged size is the output size.
//               <true>: one thread = 4 channels (16-byte loads and stores; C a multiple of 4); <false>: one channel.
#include "vd3d_dev.h"
#include "vd3d_dp_taps.h"
#include "vd3d_kernels.h"

struct dp_pyramid { int n[3], stride[3]; long long first[3]; };   // per level (full, half, quarter): patches per side, stride, index of its first patch

VD_DEV float dp_cell(float a, float b, float c, float d) { return 0.25f * ((a + b) + (c + d)); }

template <bool VEC>
__global__ __launch_bounds__(256) void k_dp_patches(const float* __restrict__ x, int B, int S, int p, dp_pyramid py, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int pw = VEC ? p >> 2 : p;                 // work items per patch row
  const int xi = (int)(idx % pw) * (VEC ? 4 : 1);
  long long r = idx / pw;
  const int y = (int)(r % p);
  const long long patch = r / p;
  const int lv = patch >= py.first[2] ? 2 : (patch >= py.first[1] ? 1 : 0);
  const long long local = patch - py.first[lv];
  const int b = (int)(local % B), l = (int)(local / B);
  const int sy = (l / py.n[lv]) * py.stride[lv] + y, sx = (l % py.n[lv]) * py.stride[lv] + xi;   // in the level's own image
  const size_t plane = (size_t)S * S;
  const float* xb = x + (size_t)b * 3 * plane;
  float* o = out + ((size_t)patch * p * p + (size_t)y * p + xi) * 3;
  if (VEC) {
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* xc = xb + c * plane;
      if (lv == 0) {
        const float4 a = *reinterpret_cast<const float4*>(xc + (size_t)sy * S + sx);
        v[c][0] = a.x; v[c][1] = a.y; v[c][2] = a.z; v[c][3] = a.w;
      } else if (lv == 1) {
        const float* r0 = xc + (size_t)(2 * sy) * S + 2 * sx;
        const float4 t0 = *reinterpret_cast<const float4*>(r0), t1 = *reinterpret_cast<const float4*>(r0 + 4);
        const float4 u0 = *reinterpret_cast<const float4*>(r0 + S), u1 = *reinterpret_cast<const float4*>(r0 + S + 4);
        v[c][0] = dp_cell(t0.x, t0.y, u0.x, u0.y); v[c][1] = dp_cell(t0.z, t0.w, u0.z, u0.w);
        v[c][2] = dp_cell(t1.x, t1.y, u1.x, u1.y); v[c][3] = dp_cell(t1.z, t1.w, u1.z, u1.w);
      } else {
        const float* r0 = xc + (size_t)(4 * sy + 1) * S + 4 * sx;
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // the cell's 16 bytes are loaded whole; its two middle pixels are used
          const float4 t = *reinterpret_cast<const float4*>(r0 + 4 * e), u = *reinterpret_cast<const float4*>(r0 + S + 4 * e);
          v[c][e] = dp_cell(t.y, t.z, u.y, u.z);
        }
      }
    }
    float4* o4 = reinterpret_cast<float4*>(o);
    o4[0] = float4{v[0][0], v[1][0], v[2][0], v[0][1]};
    o4[1] = float4{v[1][1], v[2][1], v[0][2], v[1][2]};
    o4[2] = float4{v[2][2], v[0][3], v[1][3], v[2][3]};
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* xc = xb + c * plane;
      if (lv == 0) {
        o[c] = xc[(size_t)sy * S + sx];
      } else {
        const int k = lv == 1 ? 2 : 4, off = lv == 1 ? 0 : 1;
        const float* r0 = xc + (size_t)(k * sy + off) * S + k * sx + off;
        o[c] = dp_cell(r0[0], r0[1], r0[S], r0[S + 1]);
      }
    }
  }
}

// Patches per side of a level whose image has side s: one where the image is the patch, else (s - p) / stride + 1 (split_to_patches).  0: no patch fits.
static int dp_level_patches(int s, int p, int stride) { return s < p ? 0 : (s == p ? 1 : (stride < 1 ? 0 : (s - p) / stride + 1)); }

long long vd_depthpro_patches_count(int S, int p, int stride_full, int stride_half, int stride_quarter) {
  if (S < 4 || S % 4 || p < 1) return -1;
  const int n0 = dp_level_patches(S, p, stride_full), n1 = dp_level_patches(S / 2, p, stride_half), n2 = dp_level_patches(S / 4, p, stride_quarter);
  if (n0 < 1 || n1 < 1 || n2 < 1) return -1;
  return (long long)n0 * n0 + (long long)n1 * n1 + (long long)n2 * n2;
}

// The caller has checked the shapes (vd_depthpro_patches_count >= 1) and 4-byte alignment.  false = nothing launched: a grid past 2^31 - 1 workgroups.
bool vd_launch_depthpro_patches_f32(hipStream_t s, const float* x, int B, int S, int p, int stride_full, int stride_half, int stride_quarter, float* out) {
  dp_pyramid py;
  const int side[3] = {S, S / 2, S / 4}, stride[3] = {stride_full, stride_half, stride_quarter};
  long long first = 0;
  bool vec = p % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  for (int i = 0; i < 3; ++i) {
    py.n[i] = dp_level_patches(side[i], p, stride[i]);
    py.stride[i] = py.n[i] > 1 ? stride[i] : 0;   // a level of one patch starts at the origin whatever stride was given
    py.first[i] = first;
    first += (long long)py.n[i] * py.n[i] * B;
    if (py.stride[i] % 4) vec = false;
  }
  const long long total = first * p * (vec ? p / 4 : p);
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  const dim3 g((unsigned)((total + 255) / 256)), blk(256);
  if (vec) hipLaunchKernelGGL(k_dp_patches<true>, g, blk, 0, s, x, B, S, p, py, total, out);
  else hipLaunchKernelGGL(k_dp_patches<false>, g, blk, 0, s, x, B, S, p, py, total, out);
  return true;
}

struct dp_merge { int B, T, C, g, side, pad, M, oh, ow, resize; float sy, sx; };

// merged coordinate (one axis) -> patch index k and token index t: the first patch keeps tokens [0, g - pad), the inner ones [pad, g - pad), the last [pad, g)
VD_DEV void dp_merge_index(int m, const dp_merge& q, int* k, int* t) {
  const int head = q.g - q.pad, inner = q.g - 2 * q.pad;
  if (q.side == 1 || m < head) { *k = 0; *t = m; return; }
  int kk = 1 + (m - head) / inner;
  kk = kk < q.side - 1 ? kk : q.side - 1;
  *k = kk; *t = m - (head + (kk - 1) * inner) + q.pad;
}
// offset (in floats) of the token row at merged position (my, mx) of frame b
VD_DEV size_t dp_merge_row(int my, int mx, int b, const dp_merge& q) {
  int ky, ty, kx, tx;
  dp_merge_index(my, q, &ky, &ty);
  dp_merge_index(mx, q, &kx, &tx);
  const size_t seq = (size_t)(ky * q.side + kx) * q.B + b;
  return (seq * q.T + (size_t)(q.T - q.g * q.g + ty * q.g + tx)) * q.C;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_dp_merge(const float* __restrict__ rows, dp_merge q, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cw = VEC ? q.C >> 2 : q.C;
  const int c = (int)(idx % cw) * (VEC ? 4 : 1);
  long long r = idx / cw;
  const int ox = (int)(r % q.ow);
  r /= q.ow;
  const int oy = (int)(r % q.oh), b = (int)(r / q.oh);
  float* o = out + (size_t)idx * (VEC ? 4 : 1);
  if (!q.resize) {
    const float* v = rows + dp_merge_row(oy, ox, b, q) + c;
    if (VEC) *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(v);
    else *o = *v;
    return;
  }
  const dp_tap ty = dp_linear_tap(oy, q.M, q.oh, q.sy), tx = dp_linear_tap(ox, q.M, q.ow, q.sx);
  const float* p00 = rows + dp_merge_row(ty.i0, tx.i0, b, q) + c;
  const float* p01 = rows + dp_merge_row(ty.i0, tx.i1, b, q) + c;
  const float* p10 = rows + dp_merge_row(ty.i1, tx.i0, b, q) + c;
  const float* p11 = rows + dp_merge_row(ty.i1, tx.i1, b, q) + c;
  if (VEC) {
    const float4 a = *reinterpret_cast<const float4*>(p00), bb = *reinterpret_cast<const float4*>(p01);
    const float4 cc = *reinterpret_cast<const float4*>(p10), d = *reinterpret_cast<const float4*>(p11);
    *reinterpret_cast<float4*>(o) = float4{dp_blend(ty, tx, a.x, bb.x, cc.x, d.x), dp_blend(ty, tx, a.y, bb.y, cc.y, d.y),
                                           dp_blend(ty, tx, a.z, bb.z, cc.z, d.z), dp_blend(ty, tx, a.w, bb.w, cc.w, d.w)};
  } else {
    *o = dp_blend(ty, tx, *p00, *p01, *p10, *p11);
  }
}

// merge_patches' own rules for n sequences per frame on a g x g token grid: side = int(sqrt(n)), pad = min(g / 4, padding), forced to 0 below four patches; one
// sequence is left as it is.  Returns the merged size.
int vd_depthpro_merge_geometry(int n, int g, int padding, int* side, int* pad) {
  int s = 1;
  while ((long long)(s + 1) * (s + 1) <= n) ++s;
  *side = n == 1 ? 1 : s;
  *pad = n < 4 ? 0 : (g / 4 < padding ? g / 4 : padding);
  return *side * g - 2 * *pad * (*side - 1);
}

// The caller has checked the shapes and 4-byte alignment.  false = nothing launched: a grid past 2^31 - 1 workgroups.
bool vd_launch_depthpro_merge_f32(hipStream_t s, const float* rows, int n, int B, int T, int C, int g, int padding, int oh, int ow, float* out) {
  dp_merge q;
  q.B = B; q.T = T; q.C = C; q.g = g; q.oh = oh; q.ow = ow;
  q.M = vd_depthpro_merge_geometry(n, g, padding, &q.side, &q.pad);
  q.resize = !(q.M == oh && q.M == ow);
  q.sy = (float)q.M / (float)oh; q.sx = (float)q.M / (float)ow;
  const bool vec = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const long long total = (long long)B * oh * ow * (vec ? C / 4 : C);
  if ((total + 255) / 256 > 0x7fffffffLL) return false;
  const dim3 gr((unsigned)((total + 255) / 256)), blk(256);
  if (vec) hipLaunchKernelGGL(k_dp_merge<true>, gr, blk, 0, s, rows, q, total, out);
  else hipLaunchKernelGGL(k_dp_merge<false>, gr, blk, 0, s, rows, q, total, out);
  return true;
}
