// vd3d_head_gather.hip -- the float32 head's up-sampling + head.conv2 (3 x 3, C_IN -> 32, zero padding) + tail as "coarse GEMM + fine gather" in ONE launch.
//
// Nothing non-linear sits between the bias of conv1, the align_corners bilinear up-sampling U and conv2's taps W_t, so with S_t the shift of tap t on the FINE grid
//     conv2(U(y1 + b1)) = sum over the 9 taps t of  S_t U( W_t y1 + W_t b1 )
// (vd3d_head_upconv.hip's identity).  All channel mixing happens on the COARSE map, Z_t[p][o] = sum_c W_t[o][c] y1[p][c] + bc[t][o] with bc[t][o] = sum_c W_t[o][c] b1[c]
// (depth.py head_conv2_compose): C_IN -> 9 x 32 channels on a third of the fine map's pixels.  Written to memory Z would cost more than the flops it saves, so
// a workgroup produces the Z of the coarse pixels its fine tile reaches and consumes it from LDS, one tap at a time.
//
// Arithmetic contract (restated in tests/test_head_gather_host.py):
//   Z_t[p][o]: ONE fmaf chain from 0 over the channels in the order  q = 0 .. C_IN / 8 - 1, j = 0 .. 3:  channel 8 q + j, then channel 8 q + 4 + j
//              (v_mfma_f32_32x32x2_f32 sums k = 0, then k = 1), then + bc[t][o]: one more rounding.
//   a[Y][X][o]: ONE chain acc = 0; acc = fmaf(w, z, acc) over the taps t = 3 ky + kx ascending whose fine position (Y + ky - 1, X + kx - 1) lies inside
//              [0, oh) x [0, ow) (a tap outside contributes nothing, bias included), corners (y0, x0), (y0, x1), (y1, x0), (y1, x1), corner weights the rounded
//              products ly * lx of upsample_bilinear_f32_body's coordinates (s = (float)(ih - 1) / (float)(oh - 1), f = s * (float)y, i0 = (int)f,
//              i1 = i0 + (i0 < ih - 1), l1 = f - (float)i0, l0 = 1.f - l1): hu_taps' order in vd3d_head_upconv.hip.
//   tail:      s = 0; s = fmaf(max(a[o] + b2[o], 0), w3[o], s) for o = 0 .. 31 ascending;  out = max(s + b3, 0) * scale.
// Every value is summed by one lane in one fixed order: no split-K, no atomics; bits depend neither on the batch nor on the call.
//
// Work split: a workgroup of 512 threads (8 waves, one per CU) owns one fine tile of th x tw <= TH x 32 pixels.  The coarse window the tile's 3 x 3 windows reach
// (tile + 1 fine pixel around it, + 1 coarse pixel of bilinear support: at most CY x CX pixels) is cut into groups of 32 pixels; a wave loads the y1 rows of its
// NG groups ONCE from global memory and keeps them in registers as the MFMA's A operand for all nine taps (lane = pixel lane & 31, k half lane >> 5: 16 bytes of
// channels 8 q + 4 (lane >> 5) .. + 3 per q).  Per tap: C_IN / 2 MFMAs per group with the tap's weights as B operand (LDS image [q][lane][4 floats], streamed from
// global memory a tap ahead, double-buffered), + bc, stored to the LDS buffer Z[pixel][32 channels] (rows of 36 floats: the gather's 16-byte reads of neighbouring
// pixels fall on different banks), double-buffered.  The gather of tap t - 1 runs in the same barrier interval as the MFMAs of tap t, behind them in every wave: the two waves of a SIMD drift
// apart, and one reads LDS while the other has the matrix pipe (letting waves 4 .. 7 gather first measured slower, profiles/r27_head_conv2_gather.md).  A wave's
// groups run one after the other, C_IN / 2 dependent MFMAs each (the pipe's own rate; 16 accumulator registers).  A lane owns PPL whole fine pixels
// with 32 accumulators each: per tap 4 corners x 8 ds_read_b128 and 128 FMAs per pixel, then the tail in the lane: one float stored per pixel.
// The host fits the tile to the map (whole-map exact search with the kernel's own float operations), balances it against the ragged last row and column, and
// refuses a ratio no tile serves.
//   C_IN 32 | 64:  TH 32, window 21 x 21, NG 2, PPL 2;   C_IN 128:  TH 16, window 12 x 21, NG 1, PPL 1 (the A operand is C_IN / 2 registers per group).
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include "vd3d_x3.h"
#include <type_traits>

typedef float hg_f4 __attribute__((ext_vector_type(4)));

#define HG_NT 512
#define HG_TW 32
#define HG_CX 21
#define HG_ZLD 36   // floats per Z row
__host__ __device__ constexpr int hg_th(int cin) { return cin == 128 ? 16 : 32; }
__host__ __device__ constexpr int hg_cy(int cin) { return cin == 128 ? 12 : 21; }
__host__ __device__ constexpr int hg_ng(int cin) { return cin == 128 ? 1 : 2; }
__host__ __device__ constexpr int hg_ppl(int cin) { return cin == 128 ? 1 : 2; }
__host__ __device__ constexpr int hg_zrows(int cin) { return (hg_cy(cin) * HG_CX + 31) / 32 * 32; }              // 448 | 256
__host__ __device__ constexpr int hg_zbuf(int cin) { return hg_zrows(cin) * HG_ZLD * 4; }                        // 64 512 | 36 864
__host__ __device__ constexpr int hg_wbuf(int cin) { return cin * 128; }                                         // one tap: C_IN x 32 floats
__host__ __device__ constexpr int hg_tab() { return 8 * (32 + 2) * 4; }                                          // row / column tables
__host__ __device__ constexpr int hg_lds(int cin) { return 2 * hg_zbuf(cin) + 2 * hg_wbuf(cin) + hg_tab(); }
static_assert(hg_lds(64) == 146496 && hg_lds(32) == 138304 && hg_lds(128) == 107584 && hg_lds(64) <= 160 * 1024, "LDS plan");
static_assert(hg_zrows(64) <= 8 * 32 * hg_ng(64) && hg_zrows(128) <= 8 * 32 * hg_ng(128) && hg_th(64) * HG_TW <= HG_NT * hg_ppl(64) && hg_th(128) * HG_TW <= HG_NT * hg_ppl(128), "work split");

struct vd_hg_args {
  int ih, iw, oh, ow;    // coarse / fine map
  int th, tw;            // the tile the host fitted
  int nty, ntx;          // tiles per frame column / row
  float sh, sw;
  float b3, scale;
};

template <int C_IN>
__global__ __launch_bounds__(HG_NT) void k_head_conv_gather_f32(const float* __restrict__ y1, const float* __restrict__ Wimg, const float* __restrict__ bc,
                                                               const float* __restrict__ b2, const float* __restrict__ w3, float* __restrict__ out, vd_hg_args a) {
  constexpr int NQ = C_IN / 8, NG = hg_ng(C_IN), PPL = hg_ppl(C_IN), CY = hg_cy(C_IN), ZBUF = hg_zbuf(C_IN), WBUF = hg_wbuf(C_IN);
  constexpr int W_ITEMS = WBUF / 16, W_ITERS = (W_ITEMS + HG_NT - 1) / HG_NT;
  extern __shared__ __attribute__((aligned(16))) uint8_t hg_smem[];   // the only LDS object: [Z 0][Z 1][W 0][W 1][tables]
  float* const zs = reinterpret_cast<float*>(hg_smem);
  uint8_t* const wsm = hg_smem + 2 * ZBUF;
  int* const r_o0 = reinterpret_cast<int*>(hg_smem + 2 * ZBUF + 2 * WBUF);   // corner offsets in pixels of the staged window; -1: outside the map
  int* const r_o1 = r_o0 + 34;
  int* const c_o0 = r_o0 + 68;
  int* const c_o1 = r_o0 + 102;
  float* const r_l0 = reinterpret_cast<float*>(r_o0 + 136);
  float* const r_l1 = r_l0 + 34;
  float* const c_l0 = r_l0 + 68;
  float* const c_l1 = r_l0 + 102;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kh = lane >> 5;
  const int tile = blockIdx.x;
  const int txi = tile % a.ntx, tr = tile / a.ntx, tyi = tr % a.nty, b = tr / a.nty;
  const int Y0 = tyi * a.th, X0 = txi * a.tw;
  // the coarse window: corners of the first and the last fine row / column the tile's windows reach (the coordinate is monotonic)
  const int ya = Y0 > 0 ? Y0 - 1 : 0, yb = Y0 + a.th < a.oh ? Y0 + a.th : a.oh - 1;
  const int xa = X0 > 0 ? X0 - 1 : 0, xb = X0 + a.tw < a.ow ? X0 + a.tw : a.ow - 1;
  const int cy_lo = (int)(a.sh * (float)ya), cyb = (int)(a.sh * (float)yb), cy_hi = cyb + (cyb < a.ih - 1 ? 1 : 0);
  const int cx_lo = (int)(a.sw * (float)xa), cxb = (int)(a.sw * (float)xb), cx_hi = cxb + (cxb < a.iw - 1 ? 1 : 0);
  const int ncy = cy_hi - cy_lo + 1, ncx = cx_hi - cx_lo + 1, npx = ncy * ncx;
  if (ncy > CY || ncx > HG_CX || cy_lo < 0 || cx_lo < 0 || cy_hi > a.ih - 1 || cx_hi > a.iw - 1) return;   // the host fitted the tile: never taken

  if (tid < a.th + 2) {
    const int y = Y0 - 1 + tid;
    int o0 = -1, o1 = -1;
    float l0 = 0.f, l1 = 0.f;
    if (y >= 0 && y < a.oh) {
      const float fy = a.sh * (float)y;
      const int yy0 = (int)fy;
      const int yy1 = yy0 + (yy0 < a.ih - 1 ? 1 : 0);
      l1 = fy - (float)yy0; l0 = 1.f - l1;
      o0 = (yy0 - cy_lo) * ncx; o1 = (yy1 - cy_lo) * ncx;
    }
    r_o0[tid] = o0; r_o1[tid] = o1; r_l0[tid] = l0; r_l1[tid] = l1;
  }
  if (tid >= 64 && tid < 64 + a.tw + 2) {
    const int c = tid - 64, x = X0 - 1 + c;
    int o0 = -1, o1 = -1;
    float l0 = 0.f, l1 = 0.f;
    if (x >= 0 && x < a.ow) {
      const float fx = a.sw * (float)x;
      const int xx0 = (int)fx;
      const int xx1 = xx0 + (xx0 < a.iw - 1 ? 1 : 0);
      l1 = fx - (float)xx0; l0 = 1.f - l1;
      o0 = xx0 - cx_lo; o1 = xx1 - cx_lo;
    }
    c_o0[c] = o0; c_o1[c] = o1; c_l0[c] = l0; c_l1[c] = l1;
  }

  // ---- the A operand: window pixel 32 g + li of group g = wave + 8 gi, channels 8 q + 4 kh .. + 3.  A lane past the window re-reads its last pixel (its Z rows
  // lie inside the buffer and are never read); a group past the window is skipped altogether (wave-uniform)
  const int nact = __builtin_amdgcn_readfirstlane(32 * (wave + 8 * (NG - 1)) < npx ? NG : (32 * wave < npx ? 1 : 0));
  hg_f4 areg[NG][NQ];
#pragma unroll
  for (int gi = 0; gi < NG; ++gi) {
    const int wp0 = 32 * (wave + 8 * gi) + li, wp = wp0 < npx ? wp0 : npx - 1;
    const int cyl = wp / ncx, cxl = wp - cyl * ncx;
    const float* p = y1 + (((size_t)b * a.ih + (cy_lo + cyl)) * a.iw + (cx_lo + cxl)) * C_IN + 4 * kh;
#pragma unroll
    for (int q = 0; q < NQ; ++q) areg[gi][q] = *reinterpret_cast<const hg_f4*>(p + 8 * q);
  }
  // ---- the weights of a tap: W_ITEMS 16-byte items, through registers into the LDS buffer of the tap's parity
  hg_f4 wv[W_ITERS];
  auto load_w = [&](int tap) {
#pragma unroll
    for (int p = 0; p < W_ITERS; ++p) {
      const int i = p * HG_NT + tid;
      wv[p] = *reinterpret_cast<const hg_f4*>(Wimg + (size_t)tap * (WBUF / 4) + (i < W_ITEMS ? i : W_ITEMS - 1) * 4);
    }
  };
  auto put_w = [&](int buf) {
#pragma unroll
    for (int p = 0; p < W_ITERS; ++p) {
      const int i = p * HG_NT + tid;
      if (i < W_ITEMS) *reinterpret_cast<hg_f4*>(wsm + buf * WBUF + i * 16) = wv[p];
    }
  };

  // ---- the fine pixels of this lane
  int p_ty[PPL], p_tx[PPL];
  bool p_ok[PPL];
  float acc[PPL][32];
#pragma unroll
  for (int u = 0; u < PPL; ++u) {
    const int it = u * HG_NT + tid;
    const bool in = it < a.th * a.tw;
    const int ty = in ? it / a.tw : 0, tx = in ? it - ty * a.tw : 0;
    p_ty[u] = ty; p_tx[u] = tx;
    p_ok[u] = in && Y0 + ty < a.oh && X0 + tx < a.ow;
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[u][c] = 0.f;
  }

  // one corner k = 2 (row y1) + (column x1) of tap (ky, kx) for the lane's pixel u, from the Z buffer zb: eight 16-byte reads, 32 steps of the pixel's chains
  auto gather_piece = [&](const float* zb, int ky, int kx, int u, int k) {
    const int ri = p_ty[u] + ky, ci = p_tx[u] + kx;
    const int ro0 = r_o0[ri], co0 = c_o0[ci];
    if (p_ok[u] && ro0 >= 0 && co0 >= 0) {
      const int ro = (k >> 1) ? r_o1[ri] : ro0, co = (k & 1) ? c_o1[ci] : co0;
      const float ly = (k >> 1) ? r_l1[ri] : r_l0[ri], lx = (k & 1) ? c_l1[ci] : c_l0[ci];
      const float wq = ly * lx;
      const hg_f4* zp = reinterpret_cast<const hg_f4*>(zb + (ro + co) * HG_ZLD);
#pragma unroll
      for (int c4 = 0; c4 < 8; ++c4) {
        const hg_f4 z = zp[c4];
        acc[u][4 * c4] = __builtin_fmaf(wq, z.x, acc[u][4 * c4]);
        acc[u][4 * c4 + 1] = __builtin_fmaf(wq, z.y, acc[u][4 * c4 + 1]);
        acc[u][4 * c4 + 2] = __builtin_fmaf(wq, z.z, acc[u][4 * c4 + 2]);
        acc[u][4 * c4 + 3] = __builtin_fmaf(wq, z.w, acc[u][4 * c4 + 3]);
      }
    }
  };
  // tap t of the lane's pixels from Z buffer t & 1
  auto gather_tap = [&](int t) {
    const float* zb = zs + (t & 1) * (ZBUF / 4);
    const int ky = t / 3, kx = t - 3 * ky;
#pragma unroll
    for (int u = 0; u < PPL; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) gather_piece(zb, ky, kx, u, k);
  };
  // Z of tap t for the wave's groups -> Z buffer t & 1
  auto mfma_tap = [&](int t, auto ngroups) {
    constexpr int N = decltype(ngroups)::value;
    const uint8_t* ws = wsm + (t & 1) * WBUF + lane * 16;
    float* zb = zs + (t & 1) * (ZBUF / 4);
    const float bias = bc[t * 32 + li];
    // one group after the other (16 accumulator registers live, not 32): its C_IN / 2 MFMAs are one dependent chain at the pipe's own rate
#pragma unroll
    for (int gi = 0; gi < N; ++gi) {
      x3_f16 d;
#pragma unroll
      for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const hg_f4 bw = *reinterpret_cast<const hg_f4*>(ws + q * 1024);
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[gi][q].x, bw.x, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[gi][q].y, bw.y, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[gi][q].z, bw.z, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[gi][q].w, bw.w, d, 0, 0, 0);
      }
      float* zg = zb + (32 * (wave + 8 * gi) + 4 * kh) * HG_ZLD + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) zg[((r & 3) + 8 * (r >> 2)) * HG_ZLD] = d[r] + bias;
    }
  };

  auto mfma_phase = [&](int t) {
    if (nact == NG) mfma_tap(t, std::integral_constant<int, NG>());
    else if (nact == 1) mfma_tap(t, std::integral_constant<int, 1>());
  };
  load_w(0);
  put_w(0);
  __syncthreads();   // the tables and tap 0's weights

  // interval t = 0 .. 9: the MFMAs of tap t (t < 9) and the gather of tap t - 1 (t > 0).  Z buffer t & 1 was last read in interval t - 1 (tap t - 2), the weight
  // buffer (t + 1) & 1 in interval t - 1: both in front of that interval's barrier.
#pragma unroll 1
  for (int t = 0; t <= 9; ++t) {
    if (t < 8) load_w(t + 1);
    // (HG_ABLATE_*: timing builds for tools/probe_head_conv2.py with one half left out; their results are wrong)
#ifndef HG_ABLATE_MFMA
    if (t < 9) mfma_phase(t);
#endif
#ifndef HG_ABLATE_GATHER
    if (t > 0) gather_tap(t - 1);
#endif
    if (t < 8) put_w((t + 1) & 1);
    __syncthreads();
  }

  // ---- the tail, in the lane
#pragma unroll
  for (int u = 0; u < PPL; ++u) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 32; ++c) s = __builtin_fmaf(fmaxf(acc[u][c] + b2[c], 0.f), w3[c], s);
    if (p_ok[u]) out[((size_t)b * a.oh + (Y0 + p_ty[u])) * a.ow + (X0 + p_tx[u])] = fmaxf(s + a.b3, 0.f) * a.scale;
  }
}

// ---- weights: the composed tap-major matrix Wt float32 [9 x 32][Cin] (row t 32 + o) -> [tap][q Cin / 8][lane 64][4 floats]: lane = 32 kh + o holds channels
// 8 q + 4 kh + 0 .. 3 of output channel o.  One thread = one 16-byte item.
__global__ __launch_bounds__(256) void k_head_conv_gather_pack(const float* __restrict__ Wt, int Cin, float4* __restrict__ img) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nq = Cin / 8;
  if (i >= 9 * nq * 64) return;
  const int l = i & 63, q = (i >> 6) % nq, tap = (i >> 6) / nq;
  const float* w = Wt + ((size_t)(tap * 32 + (l & 31))) * Cin + 8 * q + 4 * (l >> 5);
  img[i] = make_float4(w[0], w[1], w[2], w[3]);
}

// whether every tile of edge t along one axis reaches at most cap coarse pixels, inside the map (the kernel's own float operations)
static bool hg_fits(int n, int nc, float s, int t, int cap) {
  for (long long p0 = 0; p0 < n; p0 += t) {
    const int pa = p0 > 0 ? (int)p0 - 1 : 0, pb = p0 + t < n ? (int)(p0 + t) : n - 1;
    const int lo = (int)(s * (float)pa), hb = (int)(s * (float)pb), hi = hb + (hb < nc - 1 ? 1 : 0);
    if (lo < 0 || hi > nc - 1 || hi - lo + 1 > cap) return false;
  }
  return true;
}
// the tile edge: the largest t <= tmax that fits, then the smallest edge with the same number of tiles that fits too (little waste in the ragged last tile); 0: none
static int hg_fit(int n, int nc, float s, int tmax, int cap) {
  int t = tmax < n ? tmax : n;
  while (t >= 1 && !hg_fits(n, nc, s, t, cap)) --t;
  if (t < 1) return 0;
  const int nt = (n + t - 1) / t;
  for (int u = (n + nt - 1) / nt; u < t; ++u)
    if (hg_fits(n, nc, s, u, cap)) return u;
  return t;
}

static bool hg_plan(int B, int ih, int iw, int oh, int ow, int Cin, vd_hg_args& a) {
  if ((Cin != 32 && Cin != 64 && Cin != 128) || B < 1 || ih < 1 || iw < 1 || oh < 2 || ow < 2) return false;
  if ((long long)iw * Cin >= (1ll << 31)) return false;
  a.ih = ih; a.iw = iw; a.oh = oh; a.ow = ow;
  a.sh = (float)(ih - 1) / (float)(oh - 1); a.sw = (float)(iw - 1) / (float)(ow - 1);   // area_pixel_compute_scale, align_corners
  a.th = hg_fit(oh, ih, a.sh, hg_th(Cin), hg_cy(Cin)); a.tw = hg_fit(ow, iw, a.sw, HG_TW, HG_CX);
  if (a.th < 1 || a.tw < 1) return false;                                              // a down-sampling factor no tile serves
  a.nty = (oh + a.th - 1) / a.th; a.ntx = (ow + a.tw - 1) / a.tw;
  if ((long long)B * a.nty * a.ntx >= (1ll << 31)) return false;                        // the grid
  a.b3 = 0.f; a.scale = 1.f;
  return true;
}

long long vd_head_conv_gather_weight_bytes(int Cin) { return (Cin == 32 || Cin == 64 || Cin == 128) ? 9ll * 32 * Cin * 4 : -1; }

bool vd_head_conv_gather_shape_ok(int B, int ih, int iw, int oh, int ow, int Cin, int* th, int* tw) {
  vd_hg_args a;
  if (!hg_plan(B, ih, iw, oh, ow, Cin, a)) return false;
  if (th) *th = a.th;
  if (tw) *tw = a.tw;
  return true;
}

bool vd_launch_head_conv_gather_pack(hipStream_t s, const float* Wt, int Cin, void* img) {
  if (vd_head_conv_gather_weight_bytes(Cin) < 0 || (reinterpret_cast<uintptr_t>(img) & 15) || (reinterpret_cast<uintptr_t>(Wt) & 15)) return false;
  const int total = 9 * (Cin / 8) * 64;
  hipLaunchKernelGGL(k_head_conv_gather_pack, dim3((total + 255) / 256), dim3(256), 0, s, Wt, Cin, reinterpret_cast<float4*>(img));
  return true;
}

bool vd_launch_head_conv_gather_f32(hipStream_t s, const float* y1, int B, int ih, int iw, int oh, int ow, int Cin, const void* wimg, const float* bc, const float* b2,
                                    const float* w3, float b3, float scale, float* out) {
  vd_hg_args a;
  if (!hg_plan(B, ih, iw, oh, ow, Cin, a)) return false;
  a.b3 = b3; a.scale = scale;
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_head_conv_gather_f32<32>), hg_lds(32)}, {reinterpret_cast<const void*>(k_head_conv_gather_f32<64>), hg_lds(64)},
                     {reinterpret_cast<const void*>(k_head_conv_gather_f32<128>), hg_lds(128)}}, attr_set)) return false;
  const dim3 grid((unsigned)(B * a.nty * a.ntx));
  const float* wi = reinterpret_cast<const float*>(wimg);
  if (Cin == 32) hipLaunchKernelGGL((k_head_conv_gather_f32<32>), grid, dim3(HG_NT), hg_lds(32), s, y1, wi, bc, b2, w3, out, a);
  else if (Cin == 64) hipLaunchKernelGGL((k_head_conv_gather_f32<64>), grid, dim3(HG_NT), hg_lds(64), s, y1, wi, bc, b2, w3, out, a);
  else hipLaunchKernelGGL((k_head_conv_gather_f32<128>), grid, dim3(HG_NT), hg_lds(128), s, y1, wi, bc, b2, w3, out, a);
  return true;
}
