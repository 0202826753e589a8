// vd3d_tiles.hip -- tiled high-resolution depth (core/render_depth.py:62-66,102-194: infer_depth_tile + _normalize_to_u8), the
// memory-bound launches around the network:
//
//   k_tile_gather     apron crops of one shape group -> the [n][chs][cws][3] uint8 batch vd3d_depth_preprocess takes; every tile is
//                     cv2.resize(crop, (cws, chs), INTER_CUBIC) in the fixed-point arithmetic of k_resize_cubic_u8 (vd3d_cubic.h)
//   k_tile_blend      Hann-weighted blend of the tile centres as a GATHER: one thread per 4 output pixels walks the <= 4 x 4 tiles that
//                     cover them in the reference's row-major order (acc = acc + c * w, wacc = wacc + w from 0, one correctly rounded
//                     division) -- no atomics, identical from run to run.  A prediction plane whose size is not the tile's is sampled
//                     with bicubic_at (vd3d_cubic.h, the hand-off's arithmetic) inside the walk: the [n][chs][cws] planes never exist
//   k_pclip_hist/apply  _normalize_to_u8: numpy's linear-method percentiles (two neighbouring order statistics each) + min + max by an
//                     exact 4 x 8-bit radix select on order-preserving uint32 keys of the WHOLE float32 range (the DIBR chain's select,
//                     vd3d_select.hip, keys [0, 1] only: blended depth is signed and unbounded), then clip / truncate / invert
//
// Arithmetic: float32, one rounding per numpy operator (-ffp-contract=off), the fallback's denominator through double as numpy forms it.
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include "vd3d_cubic.h"

// ---- gather ----------------------------------------------------------------------------------------------------------------------
struct vd_gather_args { long long pitch, fstride; int B, H, W, n, ch, cw, chs, cws; double scale_x, scale_y; };

template <bool SAME>
__global__ __launch_bounds__(256) void k_tile_gather(const uint8_t* __restrict__ frames, const int32_t* __restrict__ origins, vd_gather_args a,
                                                     uint8_t* __restrict__ out) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), t = blockIdx.z;
  if (x >= a.cws || y >= a.chs) return;
  // the table is device data: clamp it into the frame batch instead of trusting it
  const int fb = min(max(origins[3 * t], 0), a.B - 1);
  const int oy = min(max(origins[3 * t + 1], 0), a.H - a.ch), ox = min(max(origins[3 * t + 2], 0), a.W - a.cw);
  const uint8_t* src = frames + (size_t)fb * a.fstride + (size_t)oy * a.pitch + (size_t)ox * 3;
  uint8_t* o = out + (((size_t)t * a.chs + y) * a.cws + x) * 3;
  if (SAME) {   // cv::resize copies when the sizes agree
    const uint8_t* p = src + (size_t)y * a.pitch + (size_t)x * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  } else {
    const rc_axis ax = rc_axis_make(x, a.scale_x, a.cw), ay = rc_axis_make(y, a.scale_y, a.ch);
    rc_cubic_pixel<3>(src, (size_t)a.pitch, ax, ay, o);
  }
}

bool vd_launch_tile_gather(hipStream_t s, const uint8_t* frames, long long pitch, long long fstride, int B, int H, int W, const int32_t* origins,
                           int n, int ch, int cw, int chs, int cws, uint8_t* out) {
  if (n > 65535) return false;
  vd_gather_args a;
  a.pitch = pitch; a.fstride = fstride; a.B = B; a.H = H; a.W = W; a.n = n; a.ch = ch; a.cw = cw; a.chs = chs; a.cws = cws;
  // cv::resize: inv_scale = dsize / ssize in double, scale = 1. / inv_scale
  a.scale_x = 1.0 / ((double)cws / (double)cw); a.scale_y = 1.0 / ((double)chs / (double)ch);
  dim3 g((cws + 63) / 64, (chs + 3) / 4, n);
  if (ch == chs && cw == cws) hipLaunchKernelGGL(k_tile_gather<true>, g, dim3(256), 0, s, frames, origins, a, out);
  else hipLaunchKernelGGL(k_tile_gather<false>, g, dim3(256), 0, s, frames, origins, a, out);
  return true;
}

// ---- blend -----------------------------------------------------------------------------------------------------------------------
// tile table, 8 ints per tile (row-major over the tile grid): yc0, xc0 (centre offset inside the prediction), chs, cws (the size the
// prediction stands for), ph, pw (the size it has), w_off (element offset of the tile's weight plane [y1-y0][x1-x0] in the pool), 0
struct vd_blend_args { int B, H, W, tile, core, nty, ntx; };

__global__ __launch_bounds__(256) void k_tile_blend(const float* __restrict__ pool, const long long* __restrict__ pred_off,
                                                    const int32_t* __restrict__ tab, const float* __restrict__ wpool, vd_blend_args a,
                                                    float* __restrict__ out) {
  const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (x4 >= a.W || y >= a.H) return;
  const int xl = min(x4 + 3, a.W - 1);
  // covering tiles: t * core <= p < t * core + tile
  const int ty_lo = y - a.tile + 1 > 0 ? (y - a.tile + a.core) / a.core : 0, ty_hi = y / a.core;
  const int tx_lo = x4 - a.tile + 1 > 0 ? (x4 - a.tile + a.core) / a.core : 0, tx_hi = xl / a.core;
  const int nt = a.nty * a.ntx;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, wacc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ty = ty_lo; ty <= ty_hi; ++ty) {
    const int y0 = ty * a.core, ly = y - y0;
    for (int tx = tx_lo; tx <= tx_hi; ++tx) {
      const int t = ty * a.ntx + tx;
      const int4 q0 = reinterpret_cast<const int4*>(tab)[2 * t], q1 = reinterpret_cast<const int4*>(tab)[2 * t + 1];
      const int yc0 = q0.x, xc0 = q0.y, chs = q0.z, cws = q0.w, ph = q1.x, pw = q1.y, w_off = q1.z;
      const int x0 = tx * a.core, tw = min(a.tile, a.W - x0);
      const float* plane = pool + pred_off[(size_t)b * nt + t];
      const float* wrow = wpool + (size_t)w_off + (size_t)ly * tw;
      const int py = yc0 + ly;
      const bool same = ph == chs && pw == cws;
      float cy[4] = {0.f, 0.f, 0.f, 0.f}, sw = 0.f;
      int iy = 0;
      if (!same) {
        const float ry = vd_fma((float)ph / (float)chs, (float)py + 0.5f, -0.5f);
        const float fy = floorf(ry);
        cubic_coeffs(ry - fy, cy);
        iy = (int)fy; sw = (float)pw / (float)cws;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int lx = x4 + q - x0;
        if (x4 + q < a.W && lx >= 0 && lx < tw) {
          const float w = wrow[lx];
          const int px = xc0 + lx;
          const float c = same ? plane[(size_t)min(py, ph - 1) * pw + min(px, pw - 1)] : bicubic_at(plane, ph, pw, sw, cy, iy, px);
          acc[q] = acc[q] + c * w;
          wacc[q] = wacc[q] + w;
        }
      }
    }
  }
  float r[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) r[q] = acc[q] / ((wacc[q] > 1e-8f || wacc[q] != wacc[q]) ? wacc[q] : 1e-8f);   // np.maximum(w_accum, 1e-8)
  float* o = out + ((size_t)b * a.H + y) * a.W + x4;
  if (x4 + 3 < a.W && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
    vd_f4 v = {r[0], r[1], r[2], r[3]};
    *reinterpret_cast<vd_f4*>(o) = v;
  } else {
    for (int q = 0; q < 4 && x4 + q < a.W; ++q) o[q] = r[q];
  }
}

void vd_launch_tile_blend(hipStream_t s, const float* pool, const long long* pred_off, const int32_t* tab, const float* wpool, int B, int H, int W,
                          int tile, int core, float* out) {
  vd_blend_args a;
  a.B = B; a.H = H; a.W = W; a.tile = tile; a.core = core; a.nty = (H + core - 1) / core; a.ntx = (W + core - 1) / core;
  hipLaunchKernelGGL(k_tile_blend, dim3((W + 255) / 256, (H + 3) / 4, B), dim3(256), 0, s, pool, pred_off, tab, wpool, a, out);
}

// ---- percentile-clip normalisation ---------------------------------------------------------------------------------------------
// ranks (ascending): 0 = min, 1 / 2 = the neighbours of the low percentile, 3 / 4 = those of the high one, 5 = max
struct vd_pclip_args { long long n; uint32_t rank[VD_PCLIP_NR]; float g_lo, g_hi; int invert; };

VD_DEV float pc_sanitize(float v) { return fabsf(v) < INFINITY ? v : 0.f; }   // np.nan_to_num(nan=0, posinf=0, neginf=0)
VD_DEV uint32_t pc_key(float v) {   // order-preserving; -0.0 sorts with +0.0 as in numpy
  v = pc_sanitize(v);
  uint32_t b = v == 0.f ? 0u : __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
VD_DEV float pc_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// After `npass` digits: the key prefix every rank lies under and the rank's position among the keys with that prefix, from the histograms of
// the passes before.  hist: [4][NR][256]; ranks that share a prefix share the histogram of the first of them.  256 threads; the result is in
// sp / sr [npass & 1].
VD_DEV void pc_resolve(int npass, const uint32_t* __restrict__ hist, const uint32_t* rank, uint32_t (*sp)[VD_PCLIP_NR], uint32_t (*sr)[VD_PCLIP_NR]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < VD_PCLIP_NR) { sp[0][threadIdx.x] = 0u; sr[0][threadIdx.x] = rank[threadIdx.x]; }
  __syncthreads();
  for (int q = 0; q < npass; ++q) {
    const int cur = q & 1, nxt = cur ^ 1;
    for (int r = wave; r < VD_PCLIP_NR; r += 4) {
      const uint32_t pref = sp[cur][r], rem = sr[cur][r];
      int leader = r;
      for (int r2 = r - 1; r2 >= 0; --r2) if (sp[cur][r2] == pref) leader = r2;
      const uint4 v = reinterpret_cast<const uint4*>(hist + ((size_t)(q * VD_PCLIP_NR + leader) << 8))[lane];
      const uint32_t s = v.x + v.y + v.z + v.w;
      uint32_t inc = s;
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)inc, off, 64);
        if (lane >= off) inc += u;
      }
      uint32_t lo = inc - s;
      if (rem >= lo && rem < lo + s) {
        int d = 0;
        if (rem >= lo + v.x) { lo += v.x; d = 1; if (rem >= lo + v.y) { lo += v.y; d = 2; if (rem >= lo + v.z) { lo += v.z; d = 3; } } }
        sp[nxt][r] = (pref << 8) | (uint32_t)(lane * 4 + d);
        sr[nxt][r] = rem - lo;
      }
    }
    __syncthreads();
  }
}

// pass p (0..3): histogram of digit p of the keys under each rank's prefix
__global__ __launch_bounds__(256) void k_pclip_hist(const float* __restrict__ planes, vd_pclip_args a, int p, uint32_t* __restrict__ ws) {
  __shared__ uint32_t sp[2][VD_PCLIP_NR], sr[2][VD_PCLIP_NR];
  __shared__ uint32_t lh[VD_PCLIP_NR * 256];
  const float* src = planes + (size_t)blockIdx.y * a.n;
  uint32_t* hist = ws + (size_t)blockIdx.y * VD_PCLIP_WS_WORDS;
  for (int i = threadIdx.x; i < VD_PCLIP_NR * 256; i += 256) lh[i] = 0u;
  pc_resolve(p, hist, a.rank, sp, sr);
  uint32_t pref[VD_PCLIP_NR];
  bool lead[VD_PCLIP_NR];
#pragma unroll
  for (int r = 0; r < VD_PCLIP_NR; ++r) {
    pref[r] = sp[p & 1][r]; lead[r] = true;
    for (int r2 = 0; r2 < r; ++r2) if (pref[r2] == pref[r]) lead[r] = false;
  }
  const int sh_d = 24 - 8 * p;
  auto add = [&](float v) {
    const uint32_t key = pc_key(v);
    const uint32_t top = p ? key >> (sh_d + 8) : 0u, d = (key >> sh_d) & 255u;
#pragma unroll
    for (int r = 0; r < VD_PCLIP_NR; ++r)
      if (lead[r] && top == pref[r]) atomicAdd(&lh[r * 256 + d], 1u);   // prefixes of leaders differ: one add per sample
  };
  const long long stride = (long long)gridDim.x * 256;
  if ((a.n & 3) == 0 && (reinterpret_cast<uintptr_t>(planes) & 15) == 0) {
    const long long n4 = a.n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
      const vd_f4 v = reinterpret_cast<const vd_f4*>(src)[i];
      add(v.x); add(v.y); add(v.z); add(v.w);
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) add(src[i]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < VD_PCLIP_NR * 256; i += 256) {
    const uint32_t c = lh[i];
    if (c) atomicAdd(&hist[(size_t)p * VD_PCLIP_NR * 256 + i], c);
  }
}

__global__ __launch_bounds__(256) void k_pclip_apply(const float* __restrict__ planes, vd_pclip_args a, const uint32_t* __restrict__ ws,
                                                     uint8_t* __restrict__ out, float* __restrict__ lohi) {
  __shared__ uint32_t sp[2][VD_PCLIP_NR], sr[2][VD_PCLIP_NR];
  __shared__ float s_sub, s_den;
  __shared__ int s_mode;
  const float* src = planes + (size_t)blockIdx.y * a.n;
  uint8_t* dst = out + (size_t)blockIdx.y * a.n;
  pc_resolve(4, ws + (size_t)blockIdx.y * VD_PCLIP_WS_WORDS, a.rank, sp, sr);
  if (threadIdx.x == 0) {
    float v[VD_PCLIP_NR];
    for (int r = 0; r < VD_PCLIP_NR; ++r) v[r] = pc_unkey(sp[0][r]);
    // numpy _lerp: a + (b - a) * t, and b - (b - a) * (1 - t) where t >= 0.5
    const float d_lo = v[2] - v[1], d_hi = v[4] - v[3];
    const float lo = a.g_lo >= 0.5f ? v[2] - d_lo * (1.f - a.g_lo) : v[1] + d_lo * a.g_lo;
    const float hi = a.g_hi >= 0.5f ? v[4] - d_hi * (1.f - a.g_hi) : v[3] + d_hi * a.g_hi;
    if (hi - lo < (float)1e-6) {   // min-max, or flat mid-grey; dmin / dmax are Python floats there: double arithmetic, one rounding
      const double dmin = (double)v[0], dmax = (double)v[5];
      if (dmax - dmin < 1e-6) { s_mode = 2; s_sub = 0.f; s_den = 1.f; }
      else { s_mode = 1; s_sub = v[0]; s_den = (float)(dmax - dmin + 1e-6); }
    } else { s_mode = 0; s_sub = lo; s_den = hi - lo; }
    if (lohi && blockIdx.x == 0) { lohi[2 * blockIdx.y] = lo; lohi[2 * blockIdx.y + 1] = hi; }
  }
  __syncthreads();
  const int mode = s_mode, inv = a.invert;
  const float sub = s_sub, den = s_den;
  auto u8 = [&](float v) -> uint32_t {
    uint32_t u = 128u;
    if (mode != 2) {
      float t = (pc_sanitize(v) - sub) / den;
      if (mode == 0) { t = t > 0.f ? t : 0.f; t = t < 1.f ? t : 1.f; }   // np.clip(., 0, 1)
      u = (uint32_t)(uint8_t)(int)(t * 255.0f);
    }
    return inv ? 255u - u : u;
  };
  const long long stride = (long long)gridDim.x * 256;
  if ((a.n & 3) == 0 && (reinterpret_cast<uintptr_t>(planes) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
    const long long n4 = a.n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
      const vd_f4 v = reinterpret_cast<const vd_f4*>(src)[i];
      reinterpret_cast<uint32_t*>(dst)[i] = u8(v.x) | (u8(v.y) << 8) | (u8(v.z) << 16) | (u8(v.w) << 24);
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) dst[i] = (uint8_t)u8(src[i]);
  }
}

void vd_launch_pclip_u8(hipStream_t s, const float* planes, int B, long long n, const uint32_t rank[VD_PCLIP_NR], float g_lo, float g_hi, int invert,
                        uint32_t* ws, uint8_t* out, float* lohi) {
  vd_pclip_args a;
  a.n = n; a.g_lo = g_lo; a.g_hi = g_hi; a.invert = invert;
  for (int r = 0; r < VD_PCLIP_NR; ++r) a.rank[r] = rank[r];
  (void)hipMemsetAsync(ws, 0, (size_t)B * VD_PCLIP_WS_WORDS * sizeof(uint32_t), s);
  long long gx = (n + 256 * 16 - 1) / (256 * 16);   // >= 16 samples per thread before the grid stride takes over
  gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
  for (int p = 0; p < 4; ++p) hipLaunchKernelGGL(k_pclip_hist, dim3((unsigned)gx, B), dim3(256), 0, s, planes, a, p, ws);
  hipLaunchKernelGGL(k_pclip_apply, dim3((unsigned)gx, B), dim3(256), 0, s, planes, a, ws, out, lohi);
}
