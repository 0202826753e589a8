// vd3d_handoff.hip -- depth hand-off: depth-net output -> the uint8 depth plane the DIBR stage reads.
//
// Reference: transformers' depth-estimation post-process (bicubic F.interpolate to the frame size,
// align_corners=False) followed by convert_depth_to_grayscale (core/render_depth.py:585-611: per-frame min-max,
// (norm*255).astype(uint8) truncation, optional 255-u8 at :1914-1916), then an XVID depth video on disk.
// Here: two small passes per batch, no full-resolution float plane and no disk hop:
//   pass 1  bicubic value at every output pixel -> wave/block min-max -> one atomicMin/Max per workgroup on
//           order-preserving uint keys (exact, order-independent)
//   pass 2  bicubic again (the 1.9 MB prediction stays in L2) -> normalise -> truncate -> packed uint8 stores
// Arithmetic = oracle/vd3d_oracle.c:vo_depth_handoff (float32, fixed association, no contraction).
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include "vd3d_cubic.h"   // cubic_coeffs / bicubic_at (shared with the tile blend)

struct vd_handoff_args { int B, ph, pw, H, W, invert, same; float sh, sw; };

VD_DEV uint32_t f2key(float v) { uint32_t b = __float_as_uint(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
VD_DEV float key2f(uint32_t k) { uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; return __uint_as_float(b); }

__global__ void k_handoff_init(uint32_t* mm, int B) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) { mm[3 * i] = 0xffffffffu; mm[3 * i + 1] = 0u; mm[3 * i + 2] = 0u; }
}

#define HO_ROWS 32  // rows per workgroup (4 waves x 8 rows each): ~8k pixels per atomic pair in pass 1
template <bool WRITE>
__global__ __launch_bounds__(256) void k_handoff(const float* __restrict__ pred, vd_handoff_args a, uint32_t* __restrict__ mm,
                                                 uint8_t* __restrict__ out) {
  const int b = blockIdx.z;
  const float* p = pred + (size_t)b * a.ph * a.pw;
  const int xq = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;  // 4 consecutive pixels per thread
  float bmn = INFINITY, bmx = -INFINITY;
  int bbad = 0;
  for (int ry_ = 0; ry_ < HO_ROWS / 4; ++ry_) {
  const int y = blockIdx.y * HO_ROWS + ry_ * 4 + (threadIdx.x >> 6);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const bool row_ok = y < a.H;
  if (row_ok && xq < a.W) {
    if (a.same) {
#pragma unroll
      for (int q = 0; q < 4; ++q) if (xq + q < a.W) v[q] = p[(size_t)y * a.W + xq + q];
    } else {
      const float ry = vd_fma(a.sh, (float)y + 0.5f, -0.5f);
      const float fy = floorf(ry);
      float cy[4];
      cubic_coeffs(ry - fy, cy);
#pragma unroll
      for (int q = 0; q < 4; ++q) if (xq + q < a.W) v[q] = bicubic_at(p, a.ph, a.pw, a.sw, cy, (int)fy, xq + q);
    }
  }
  if (!WRITE) {
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    if (row_ok)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (xq + q < a.W) { bad |= (v[q] != v[q]); mn = v[q] < mn ? v[q] : mn; mx = v[q] > mx ? v[q] : mx; }
    bmn = fminf(bmn, mn); bmx = fmaxf(bmx, mx); bbad |= bad;
  } else {
    if (!row_ok || xq >= a.W) continue;
    const float mn = key2f(mm[3 * b]), mx = key2f(mm[3 * b + 1]);
    const bool flat = mm[3 * b + 2] != 0u || (mx - mn) < (float)1e-6;
    const float den = (mx - mn) + (float)1e-6;
    uint32_t pack = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint8_t u = 0;
      if (!flat) {
        float n = ((v[q] - mn) / den) * 255.f;
        n = n < 0.f ? 0.f : (n > 255.f ? 255.f : n);
        u = (uint8_t)n;
      }
      if (a.invert) u = (uint8_t)(255 - u);
      pack |= (uint32_t)u << (8 * q);
    }
    uint8_t* o = out + (size_t)b * a.H * a.W + (size_t)y * a.W + xq;
    if (xq + 3 < a.W && (((size_t)b * a.H * a.W + (size_t)y * a.W + xq) & 3) == 0) *reinterpret_cast<uint32_t*>(o) = pack;
    else for (int q = 0; q < 4 && xq + q < a.W; ++q) o[q] = (uint8_t)(pack >> (8 * q));
  }
  }  // rows
  if (!WRITE) {
    __shared__ float smn[4], smx[4];
    __shared__ int sbad[4];
    for (int off = 32; off > 0; off >>= 1) {
      bmn = fminf(bmn, __shfl_down(bmn, off, 64));
      bmx = fmaxf(bmx, __shfl_down(bmx, off, 64));
      bbad |= __shfl_down(bbad, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = bmn; smx[threadIdx.x >> 6] = bmx; sbad[threadIdx.x >> 6] = bbad; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const float mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
      const float mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
      if (mn <= mx) { atomicMin(&mm[3 * b], f2key(mn)); atomicMax(&mm[3 * b + 1], f2key(mx)); }
      if (sbad[0] | sbad[1] | sbad[2] | sbad[3]) atomicOr(&mm[3 * b + 2], 1u);
    }
  }
}

// ---- the separable fast form, for up-scaling (ph <= H, pw <= W, not the identity) ---------------------------------------------------------------------
// bicubic_at evaluates r(yy, x) = (((0 + row[xs0] * cx0) + row[xs1] * cx1) + row[xs2] * cx2) + row[xs3] * cx3 for its four prediction rows yy at every
// output pixel, although r depends on the prediction row and the output column only: at x4.17 every r is computed about eleven times.  Here ONE WAVE
// walks the HO_ROWS output rows of its 64 x 4 columns.  A thread computes cx[4] / xs[4] of its four columns once and keeps r of the four unclamped
// prediction rows iy - 1 .. iy + 2 in registers; the output row is uniform over the wave, so the window moves by uniform branches: not at all, by one row
// (three moves and one new r), or it is rebuilt.  A row that the border clamp maps onto its neighbour's copies that neighbour's r.  Every r and the
// vertical sum acc = (((0 + r0 * cy0) + r1 * cy1) + r2 * cy2) + r3 * cy3 are bicubic_at's operations in bicubic_at's order: the same bits as k_handoff.
struct ho_cols { float cx[4][4]; int xs[4][4]; };
struct ho_window { float r[4][4]; int iy; bool live; };   // r[i][q]: prediction row clamp(iy - 1 + i), column q of the thread

VD_DEV void ho_cols_make(ho_cols& c, int xq, int pw, float sw) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float rx = vd_fma(sw, (float)(xq + q) + 0.5f, -0.5f);
    const float fx = floorf(rx);
    const int ix = (int)fx;
    cubic_coeffs(rx - fx, c.cx[q]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { int xx = ix - 1 + j; c.xs[q][j] = xx < 0 ? 0 : (xx > pw - 1 ? pw - 1 : xx); }
  }
}
VD_DEV void ho_hrow(const float* __restrict__ row, const ho_cols& c, float r[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) v += row[c.xs[q][j]] * c.cx[q][j];
    r[q] = v;
  }
}
VD_DEV int ho_clamp_row(int yy, int ph) { return yy < 0 ? 0 : (yy > ph - 1 ? ph - 1 : yy); }
// the four values of output row y (uniform over the wave) at the thread's columns; both passes call this, so both see the same values
VD_DEV void ho_row_values(const float* __restrict__ p, int ph, int pw, float sh, int y, const ho_cols& c, ho_window& w, float v[4]) {
  const float ry = vd_fma(sh, (float)y + 0.5f, -0.5f);
  const float fy = floorf(ry);
  const int iy = __builtin_amdgcn_readfirstlane((int)fy);
  float cy[4];
  cubic_coeffs(ry - fy, cy);
  if (w.live && iy == w.iy + 1) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) w.r[i][q] = w.r[i + 1][q];
    const int yn = ho_clamp_row(iy + 2, ph);
    if (yn != ho_clamp_row(iy + 1, ph)) ho_hrow(p + (size_t)yn * pw, c, w.r[3]);   // else: the clamped row's r, already in r[3] == r[2]
  } else if (!w.live || iy != w.iy) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int yy = ho_clamp_row(iy - 1 + i, ph);
      if (i > 0 && yy == ho_clamp_row(iy - 2 + i, ph)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) w.r[i][q] = w.r[i - 1][q];
      } else {
        ho_hrow(p + (size_t)yy * pw, c, w.r[i]);
      }
    }
  }
  w.iy = iy; w.live = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc += w.r[i][q] * cy[i];
    v[q] = acc;
  }
}

template <bool WRITE>
__global__ __launch_bounds__(64) void k_handoff_sep(const float* __restrict__ pred, vd_handoff_args a, uint32_t* __restrict__ mm,
                                                    uint8_t* __restrict__ out) {
  const int b = blockIdx.z;
  const float* p = pred + (size_t)b * a.ph * a.pw;
  const int xq = (blockIdx.x * 64 + threadIdx.x) * 4;   // 4 consecutive pixels per thread; columns past W take clamped taps and are dropped below
  ho_cols c;
  ho_cols_make(c, xq, a.pw, a.sw);
  ho_window w;
  w.iy = 0; w.live = false;
  float bmn = INFINITY, bmx = -INFINITY;
  int bbad = 0;
  float mn = 0.f, den = 1.f;
  bool flat = false;
  if (WRITE) {
    const float mx = key2f(mm[3 * b + 1]);
    mn = key2f(mm[3 * b]);
    flat = mm[3 * b + 2] != 0u || (mx - mn) < (float)1e-6;
    den = (mx - mn) + (float)1e-6;
  }
  const int y_end = min(a.H, (int)(blockIdx.y + 1) * HO_ROWS);
  for (int y = blockIdx.y * HO_ROWS; y < y_end; ++y) {
    float v[4];
    ho_row_values(p, a.ph, a.pw, a.sh, y, c, w, v);
    if (!WRITE) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (xq + q < a.W) { bbad |= (v[q] != v[q]); bmn = v[q] < bmn ? v[q] : bmn; bmx = v[q] > bmx ? v[q] : bmx; }
    } else {
      if (xq >= a.W) continue;
      uint32_t pack = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint8_t u = 0;
        if (!flat) {
          float n = ((v[q] - mn) / den) * 255.f;
          n = n < 0.f ? 0.f : (n > 255.f ? 255.f : n);
          u = (uint8_t)n;
        }
        if (a.invert) u = (uint8_t)(255 - u);
        pack |= (uint32_t)u << (8 * q);
      }
      uint8_t* o = out + (size_t)b * a.H * a.W + (size_t)y * a.W + xq;
      if (xq + 3 < a.W && (((size_t)b * a.H * a.W + (size_t)y * a.W + xq) & 3) == 0) *reinterpret_cast<uint32_t*>(o) = pack;
      else for (int q = 0; q < 4 && xq + q < a.W; ++q) o[q] = (uint8_t)(pack >> (8 * q));
    }
  }
  if (!WRITE) {
    for (int off = 32; off > 0; off >>= 1) {
      bmn = fminf(bmn, __shfl_down(bmn, off, 64));
      bmx = fmaxf(bmx, __shfl_down(bmx, off, 64));
      bbad |= __shfl_down(bbad, off, 64);
    }
    if (threadIdx.x == 0) {
      if (bmn <= bmx) { atomicMin(&mm[3 * b], f2key(bmn)); atomicMax(&mm[3 * b + 1], f2key(bmx)); }
      if (bbad) atomicOr(&mm[3 * b + 2], 1u);
    }
  }
}

// form: 0 = the separable kernel where it applies, 1 = k_handoff, 2 = the separable kernel or false
bool vd_launch_depth_handoff(hipStream_t s, const float* pred, int B, int ph, int pw, int H, int W, int invert, uint32_t* mm,
                             uint8_t* out, int form) {
  vd_handoff_args a;
  a.B = B; a.ph = ph; a.pw = pw; a.H = H; a.W = W; a.invert = invert; a.same = (ph == H && pw == W);
  a.sh = (float)ph / (float)H; a.sw = (float)pw / (float)W;
  const bool sep_ok = !a.same && ph <= H && pw <= W;
  if (form == 2 && !sep_ok) return false;
  hipLaunchKernelGGL(k_handoff_init, dim3((B + 63) / 64), dim3(64), 0, s, mm, B);
  dim3 g((W + 255) / 256, (H + HO_ROWS - 1) / HO_ROWS, B);
  if (form != 1 && sep_ok) {
    hipLaunchKernelGGL(k_handoff_sep<false>, g, dim3(64), 0, s, pred, a, mm, out);
    hipLaunchKernelGGL(k_handoff_sep<true>, g, dim3(64), 0, s, pred, a, mm, out);
    return true;
  }
  hipLaunchKernelGGL(k_handoff<false>, g, dim3(256), 0, s, pred, a, mm, out);
  hipLaunchKernelGGL(k_handoff<true>, g, dim3(256), 0, s, pred, a, mm, out);
  return true;
}
