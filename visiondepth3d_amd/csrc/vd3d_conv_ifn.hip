// vd3d_conv_ifn.hip -- the float32 glue between the blocks of the RIFE interpolation network (IFNet HDv3): warp + down-scale + concatenate (the 16-channel input
// of an IFBlock), the flow / mask update behind its last transposed convolution, and the final blend.  The network's convolutions (vd3d_conv_ifn) are the tile
// kernel of vd3d_conv_x3.hip.
#include "vd3d_dev.h"
#include "vd3d_kernels.h"

// Float32 glue of the interpolation network.  X: the network input, planar [N][6][h][w] (two frames in [0, 1]); the network works on the size padded
// with zeros to Hp x Wp (multiples of 32): a pixel outside h x w reads 0.  S: the running state, NHWC [N][Hp][Wp][8] = flow (4), mask (1), zeros (3).
// The warp is grid_sample(align_corners=True, padding_mode="border") in pixel units: a bilinear sample at pixel + flow clamped to [0, Wp-1] x [0, Hp-1].
// Every index is clamped into the padded frame before it is used, whatever the flow holds (Inf, NaN, 1e30).
struct rf_img { const float* p; int h, w, Hp, Wp; };
__device__ __forceinline__ float rf_px(const rf_img& im, int c, int y, int x) {
  return (y < im.h && x < im.w) ? im.p[((size_t)c * im.h + y) * im.w + x] : 0.f;
}
// one axis of the sample position x + f, clamped to [0, n - 1], as (left index, fraction): the integer part of f is added in integers, so the position is exact
__device__ __forceinline__ void rf_axis(int x, float f, int n, int& i0, int& i1, float& a) {
  const float fi = floorf(fminf(fmaxf(f, -65536.f), 65536.f));   // NaN -> -65536: clamps to the left border
  const int i = x + (int)fi;
  a = (i < 0 || i >= n - 1 || !(f == f)) ? 0.f : f - fi;
  i0 = min(max(i, 0), n - 1);
  i1 = min(i0 + 1, n - 1);
}
__device__ __forceinline__ void rf_warp3(const rf_img& im, int c0, int x, int y, float fx, float fy, float out[3]) {
  int xa, xb2, ya, yb2; float ax, ay;
  rf_axis(x, fx, im.Wp, xa, xb2, ax);
  rf_axis(y, fy, im.Hp, ya, yb2, ay);
  const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    out[c] = rf_px(im, c0 + c, ya, xa) * w00 + rf_px(im, c0 + c, ya, xb2) * w01 + rf_px(im, c0 + c, yb2, xa) * w10 + rf_px(im, c0 + c, yb2, xb2) * w11;
}
// the 11 values of one full-size pixel: warped frame 0 (3), warped frame 1 (3), mask, flow (4)
__device__ __forceinline__ void rf_pixel11(const rf_img& im, const float* S, int first, int n, int y, int x, float v[11]) {
  float4 fl = make_float4(0.f, 0.f, 0.f, 0.f); float mk = 0.f;
  if (!first) {
    const float* sp = S + (((size_t)n * im.Hp + y) * im.Wp + x) * 8;
    fl = *reinterpret_cast<const float4*>(sp); mk = sp[4];
  }
  rf_warp3(im, 0, x, y, fl.x, fl.y, v);
  rf_warp3(im, 3, x, y, fl.z, fl.w, v + 3);
  v[6] = mk; v[7] = fl.x; v[8] = fl.y; v[9] = fl.z; v[10] = fl.w;
}

// One block's 16-channel input at 1/s: F.interpolate(scale_factor=1/s, bilinear, align_corners=False) of sizes that are multiples of s is the mean of the two
// centre pixels of each s-cell per axis, so only the centre 2 x 2 of a cell is warped.  out NHWC [N][Hp/s][Wp/s][16] = 7 image channels, flow / s, 5 zeros.
__global__ __launch_bounds__(256) void k_rife_warp_pack(const float* __restrict__ X, const float* __restrict__ S, int first, int h, int w, int Hp, int Wp,
                                                        int s, float* __restrict__ out) {
  const int hs = Hp / s, ws = Wp / s, n = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hs * ws) return;
  const int dy = i / ws, dx = i - dy * ws;
  const rf_img im{X + (size_t)n * 6 * h * w, h, w, Hp, Wp};
  float v[11];
  if (s == 1) rf_pixel11(im, S, first, n, dy, dx, v);
  else {
    const int cy = s * dy + s / 2 - 1, cx = s * dx + s / 2 - 1;
    float a00[11], a01[11], a10[11], a11[11];
    rf_pixel11(im, S, first, n, cy, cx, a00); rf_pixel11(im, S, first, n, cy, cx + 1, a01);
    rf_pixel11(im, S, first, n, cy + 1, cx, a10); rf_pixel11(im, S, first, n, cy + 1, cx + 1, a11);
#pragma unroll
    for (int k = 0; k < 11; ++k) v[k] = 0.5f * (0.5f * a00[k] + 0.5f * a01[k]) + 0.5f * (0.5f * a10[k] + 0.5f * a11[k]);
  }
  const float is = 1.f / (float)s;
  float4* o = reinterpret_cast<float4*>(out + (((size_t)n * hs + dy) * ws + dx) * 16);
  o[0] = make_float4(v[0], v[1], v[2], v[3]);
  o[1] = make_float4(v[4], v[5], v[6], v[7] * is);
  o[2] = make_float4(v[8] * is, v[9] * is, v[10] * is, 0.f);
  o[3] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// flow += up(T[..0:4]) * s, mask += up(T[..4]); up = F.interpolate(scale_factor=s, bilinear, align_corners=False): source (d + 0.5) / s - 0.5 clamped at 0.
// T: NHWC [N][Hp/s][Wp/s] pixels of pitch t_stride (the last transposed convolution's output, 5 real channels).  first: S = instead of S +=.
__global__ __launch_bounds__(256) void k_rife_update(const float* __restrict__ T, int t_stride, int first, int Hp, int Wp, int s, float* __restrict__ S) {
  const int n = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Hp * Wp) return;
  const int y = i / Wp, x = i - y * Wp, hs = Hp / s, ws = Wp / s;
  const float rs = 1.f / (float)s;
  const float syf = fmaxf(((float)y + 0.5f) * rs - 0.5f, 0.f), sxf = fmaxf(((float)x + 0.5f) * rs - 0.5f, 0.f);
  const int ya = min((int)syf, hs - 1), xa = min((int)sxf, ws - 1), yb2 = min(ya + 1, hs - 1), xb2 = min(xa + 1, ws - 1);
  const float ly = syf - (float)ya, lx = sxf - (float)xa, hy = 1.f - ly, hx = 1.f - lx;
  const float* t0 = T + (size_t)n * hs * ws * t_stride;
  const float* p00 = t0 + ((size_t)ya * ws + xa) * t_stride; const float* p01 = t0 + ((size_t)ya * ws + xb2) * t_stride;
  const float* p10 = t0 + ((size_t)yb2 * ws + xa) * t_stride; const float* p11 = t0 + ((size_t)yb2 * ws + xb2) * t_stride;
  float* sp = S + (((size_t)n * Hp + y) * Wp + x) * 8;
  float o[8];
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    float u = hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]);
    if (c < 4) u = u * (float)s;
    o[c] = first ? u : sp[c] + u;
  }
  o[5] = o[6] = o[7] = 0.f;
  reinterpret_cast<float4*>(sp)[0] = make_float4(o[0], o[1], o[2], o[3]);
  reinterpret_cast<float4*>(sp)[1] = make_float4(o[4], o[5], o[6], o[7]);
}

// out planar [N][3][h][w] = warp(frame 0, flow[0:2]) * m + warp(frame 1, flow[2:4]) * (1 - m), m = sigmoid(mask); the 32-padding is cropped
__global__ __launch_bounds__(256) void k_rife_blend(const float* __restrict__ X, const float* __restrict__ S, int h, int w, int Hp, int Wp, float* __restrict__ out) {
  const int n = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  const rf_img im{X + (size_t)n * 6 * h * w, h, w, Hp, Wp};
  float v[11];
  rf_pixel11(im, S, 0, n, y, x, v);
  const float m = 1.f / (1.f + expf(-v[6]));
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(((size_t)n * 3 + c) * h + y) * w + x] = v[c] * m + v[3 + c] * (1.f - m);
}

void vd_launch_rife_warp_pack(hipStream_t s, const float* X, const float* S, int first, int N, int h, int w, int Hp, int Wp, int scale, float* out) {
  const int npix = (Hp / scale) * (Wp / scale);
  hipLaunchKernelGGL(k_rife_warp_pack, dim3((npix + 255) / 256, N), dim3(256), 0, s, X, S, first, h, w, Hp, Wp, scale, out);
}
void vd_launch_rife_update(hipStream_t s, const float* T, int t_stride, int first, int N, int Hp, int Wp, int scale, float* S) {
  hipLaunchKernelGGL(k_rife_update, dim3((Hp * Wp + 255) / 256, N), dim3(256), 0, s, T, t_stride, first, Hp, Wp, scale, S);
}
void vd_launch_rife_blend(hipStream_t s, const float* X, const float* S, int N, int h, int w, int Hp, int Wp, float* out) {
  hipLaunchKernelGGL(k_rife_blend, dim3((h * w + 255) / 256, N), dim3(256), 0, s, X, S, h, w, Hp, Wp, out);
}
