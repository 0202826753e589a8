// vd3d_conv_rdb.hip -- the convolutions of RealESRGAN_x4plus (RRDBNet, 23 residual-in-residual dense blocks): 3x3, stride 1, zero padding 1,
// C_in in {64, 96, 128, 160, 192} -> C_out in {32, 64}, fp16 in / fp16 out / float32 accumulate on v_mfma_f32_32x32x16_f16 -- the arithmetic
// of k_conv3x3_c64_s (vd3d_conv.hip), generalised in three directions:
//   * STRIDED CHANNEL SLICES.  The input is the first C_in channels of an NHWC buffer with a pixel stride of x_stride channels, the output is
//     the C_out channels at offset y_offset of a buffer with pixel stride y_stride -- which may be the SAME buffer: a dense block keeps
//     x | conv1 | conv2 | conv3 | conv4 in one [H][W][192] buffer, every convolution reads a prefix and writes the next slice, and the four
//     torch.cat of the module graph do not exist.  Read and written channels are disjoint in whole 16-byte pieces, so no workgroup's halo
//     read touches a byte another workgroup writes (the entry point refuses an intersecting slice).
//   * K STREAMED THROUGH LDS.  The 192-channel tile of a 34 x 10 window is 130 KB; the channels pass through a ring of TWO stages of 32
//     channels each (4 chunk planes of 340 pixels x 16 B, pitch 5 664 B == 32 mod 256, the conflict-free ds_read_b128 layout of vd3d_conv.hip):
//     while the waves multiply stage c & 1, the next 32 channels travel from global memory into registers (6 x 16 B per thread) and are
//     written to stage (c + 1) & 1 behind the MFMAs; ONE barrier per 32 channels.  The accumulators live across the whole K loop.
//   * A RESIDUAL EPILOGUE in float32: v = acc + bias; v = v >= 0 ? v : v * slope; v = v * alpha + r1 (if r1); v = v * beta + r2 (if r2); ONE
//     fp16 rounding at the store.  conv5 of an RDB is (alpha 0.2, r1 = x), conv5 of an RRDB's third RDB (0.2, x_rdb, 0.2, x_rrdb), conv_body
//     (1, feat).  Multiply and add are separate float32 roundings (-ffp-contract=off), like the module graph's `conv * 0.2 + x` in float32.
//   * up2 (64 -> 64 only): tap (gy, gx) reads pixel (gy >> 1, gx >> 1) of an input of half the size; padding is tested against the
//     up-sampled size.  F.interpolate(scale_factor=2, mode="nearest") in front of conv_up1 / conv_up2 is folded into the tile load.
// Tile order: a 1-D grid walks the 32 x 8 tiles so that every XCD owns one contiguous band of them (vd_xcd_tile): the halo rows two vertically adjacent
//   tiles share are found in the XCD's own L2 (measured against the row-major 2-D grid: 44.0 -> 38.3 us for 64 -> 32 at 960 x 540, 45.3 -> 43.8 ms per frame).
// Work split: a workgroup = a 32 x 8 output tile, 256 threads = 4 waves.  C_out 64: wave = (row half, channel tile), 4 rows x 1 channel tile
//   (64 accumulator registers, every weight fragment feeds 4 MFMAs).  C_out 32: wave = 2 rows of the one channel tile (32 accumulator registers).
// K ORDER (fixed; the kernel is bit-for-bit repeatable -- no atomics, no order that depends on scheduling): for chunk c = 0 .. C_in/32 - 1,
//   for tap = kh*3 + kw = 0 .. 8, for kc = 0, 1: one MFMA step over channels 32c + 16kc .. + 15, i.e. step = (c*9 + tap)*2 + kc.
// Weights: fragment image [C_in/32 * 18 steps][C_out/32][64 lanes][8 halves], element [step][t][l][j] = Wt[32t + (l & 31)][32c + 16kc + 8(l >> 5) + j][kh][kw]
//   (upscale.dense_weight_fragments), streamed from global memory two steps ahead of use; L2-resident (C_in 192, C_out 64: 221 KB).
// LDS: the ring (2 x 22 656 B) + bias[64] float32 = 45 568 B dynamic, no static LDS: THREE workgroups per CU (136.7 of 160 KB), which needs
//   <= 168 registers per lane (12 waves per CU = 3 per SIMD of 512); the epilogue reuses the ring as the pixel-major staging buffer
//   (pitch C_out*2 + 16 B) for 16-byte NHWC stores.
// Bounds (960 x 540): 192 -> 64 is 114.7 GFLOP -> 46 us at the 2.5 PFLOP/s dense fp16 peak; 64 -> 32 is 19.1 GFLOP (8 us) but 66 MB in (x 1.33 halo) + 33 MB out.
// Measured (tools/probe_rrdb.py, profiles/r10_rrdb.md): 192 -> 64 120 us = 952 TFLOP/s = 38 % of the peak, 2.6x MIOpen's convolution + leaky_relu; 64 -> 32 39.5 us
// = 484 TFLOP/s = 19 %, bound by its bytes (3.1 TB/s), 2.1x MIOpen; the whole network 29.1 ms at 960 x 540 against 100.0 ms for the fp16 module graph.
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include <hip/hip_fp16.h>

typedef _Float16 rd_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 rd_h4 __attribute__((ext_vector_type(4)));
typedef float rd_f16 __attribute__((ext_vector_type(16)));

#define RD_TW 32
#define RD_TH 8
#define RD_PW (RD_TW + 2)
#define RD_PH (RD_TH + 2)
#define RD_NPIX (RD_PW * RD_PH)                             // 340
#define RD_PLANE ((RD_NPIX * 16 + 255) / 256 * 256 + 32)    // 5 664 bytes per 8-channel plane
#define RD_STAGE (4 * RD_PLANE)                             // 32 channels: 22 656
#define RD_RING (2 * RD_STAGE)                              // 45 312
#define RD_LDS (RD_RING + 256)                              // + bias[64] float32
#define RD_NLD ((RD_NPIX * 4 + 255) / 256)                  // 16-byte pieces of one stage per thread: 6 (5.3)
#define RD_WD 2                                             // weight fragments are requested this many steps ahead (18 % (RD_WD + 1) == 0)

struct rd_args {
  const _Float16* x; int H, W, x_stride, nch;               // nch = C_in / 32
  const uint4* wfrag; const float* bias; float slope, alpha, beta;
  const _Float16* r1; int r1_stride; const _Float16* r2; int r2_stride;
  _Float16* y; int y_stride, y_offset;
  int ntx, ntiles, per;                                      // tile walk (vd_xcd_tile): 8 * per workgroups, XCD b % 8 owns one band of `per` tiles
};

// the 32 channels 32c .. of the (32 + 2) x (8 + 2) window -> registers (zero outside the image); thread = (piece tid & 3, pixel (tid >> 2) + 64k)
template <bool UP2>
VD_DEV void rd_issue(const rd_args& a, int x0, int y0, int c, int tid, uint4 (&v)[RD_NLD]) {
  const int piece = tid & 3, p0 = tid >> 2;
  const int sw = UP2 ? a.W >> 1 : a.W;
#pragma unroll
  for (int k = 0; k < RD_NLD; ++k) {
    const int pix = p0 + 64 * k;
    const int py = pix / RD_PW, px = pix - py * RD_PW;
    const int gy = y0 - 1 + py, gx = x0 - 1 + px;
    v[k] = make_uint4(0u, 0u, 0u, 0u);
    if (pix < RD_NPIX && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const int sy = UP2 ? gy >> 1 : gy, sx = UP2 ? gx >> 1 : gx;
      v[k] = *reinterpret_cast<const uint4*>(a.x + ((size_t)sy * sw + sx) * a.x_stride + c * 32 + piece * 8);
    }
  }
}
VD_DEV void rd_store(uint8_t* stage, int tid, const uint4 (&v)[RD_NLD]) {
  const int piece = tid & 3, p0 = tid >> 2;
#pragma unroll
  for (int k = 0; k < RD_NLD; ++k) {
    const int pix = p0 + 64 * k;
    if (pix < RD_NPIX) *reinterpret_cast<uint4*>(stage + piece * RD_PLANE + pix * 16) = v[k];
  }
}

template <int NT, bool UP2>   // NT = C_out / 32
__global__ __launch_bounds__(256, 3) void k_conv3x3_dense_f16(const rd_args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rd_lds[];
  constexpr int RW = NT == 2 ? 4 : 2;                        // tile rows per wave
  constexpr int OP = 64 * NT + 16;                           // epilogue: bytes per staged pixel
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, g = lane >> 5;
  const int tile = vd_xcd_tile(blockIdx.x, a.per, 1);
  if (tile >= a.ntiles) return;                              // padding workgroup of the last band (workgroup-uniform, before any barrier)
  const int tby = tile / a.ntx, tbx = tile - tby * a.ntx;
  const int x0 = tbx * RD_TW, y0 = tby * RD_TH;
  const int ct = NT == 2 ? (wave & 1) : 0;                   // channel tile (output channels 32 ct ..)
  const int row0 = NT == 2 ? (wave >> 1) * 4 : wave * 2;     // first tile row of this wave
  float* lbias = reinterpret_cast<float*>(rd_lds + RD_RING);
  if (tid < 32 * NT) lbias[tid] = a.bias[tid];

  const uint4* wp = a.wfrag + ct * 64 + lane;                // this wave's A fragment of step s: wp[s * 64 * NT]
  const int last_step = a.nch * 18 - 1;
  uint4 aw[RD_WD + 1];
#pragma unroll
  for (int d = 0; d < RD_WD; ++d) aw[d] = wp[d * 64 * NT];

  uint4 v[RD_NLD];
  rd_issue<UP2>(a, x0, y0, 0, tid, v);
  rd_store(rd_lds, tid, v);
  __syncthreads();

  rd_f16 acc[RW];
#pragma unroll
  for (int m = 0; m < RW; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

  for (int c = 0; c < a.nch; ++c) {
    // the next 32 channels travel while this stage is multiplied (the last iteration re-reads its own chunk -- cached, never used -- so that no
    // control flow surrounds the live prefetch registers)
    rd_issue<UP2>(a, x0, y0, c + 1 < a.nch ? c + 1 : c, tid, v);
    const uint8_t* bbase = rd_lds + (c & 1) * RD_STAGE + g * RD_PLANE + (row0 * RD_PW + li) * 16;
    rd_h8 bf[2][RW];
#pragma unroll
    for (int m = 0; m < RW; ++m) bf[0][m] = *reinterpret_cast<const rd_h8*>(bbase + m * RD_PW * 16);
#pragma unroll
    for (int s = 0; s < 18; ++s) {
      aw[(s + RD_WD) % (RD_WD + 1)] = wp[(size_t)min(c * 18 + s + RD_WD, last_step) * (64 * NT)];
      if (s + 1 < 18) {
        const int tap = (s + 1) >> 1, kc = (s + 1) & 1, dy = tap / 3, dx = tap - 3 * dy;
        const uint8_t* bp = bbase + (2 * kc) * RD_PLANE + (dy * RD_PW + dx) * 16;
#pragma unroll
        for (int m = 0; m < RW; ++m) bf[(s + 1) & 1][m] = *reinterpret_cast<const rd_h8*>(bp + m * RD_PW * 16);
      }
      const rd_h8 wa = __builtin_bit_cast(rd_h8, aw[s % (RD_WD + 1)]);
#pragma unroll
      for (int m = 0; m < RW; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, bf[s & 1][m], acc[m], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // stage (c + 1) & 1 was last read in iteration c - 1, and every wave has passed the barrier that ended it
    rd_store(rd_lds + ((c + 1) & 1) * RD_STAGE, tid, v);
    __syncthreads();
  }
  // every wave is done with the ring: it becomes the output staging buffer (256 pixels x OP bytes <= 36 864)

  // epilogue in float32, accumulator layout: lane = pixel li of tile row row0 + m; registers 4q .. 4q+3 = channels 32 ct + 8q + 4g + (0..3)
  const bool has1 = a.r1 != nullptr, has2 = a.r2 != nullptr;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ch = 32 * ct + 8 * q + 4 * g;
    const float4 bv = *reinterpret_cast<const float4*>(lbias + ch);
#pragma unroll
    for (int m = 0; m < RW; ++m) {
      const int gy = y0 + row0 + m, gx = x0 + li;
      const bool in = gy < a.H && gx < a.W;
      float v0 = acc[m][4 * q] + bv.x, v1 = acc[m][4 * q + 1] + bv.y, v2 = acc[m][4 * q + 2] + bv.z, v3 = acc[m][4 * q + 3] + bv.w;
      v0 = v0 >= 0.f ? v0 : v0 * a.slope; v1 = v1 >= 0.f ? v1 : v1 * a.slope; v2 = v2 >= 0.f ? v2 : v2 * a.slope; v3 = v3 >= 0.f ? v3 : v3 * a.slope;
      if (has1) {
        rd_h4 r = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
        if (in) r = *reinterpret_cast<const rd_h4*>(a.r1 + ((size_t)gy * a.W + gx) * a.r1_stride + ch);
        v0 = v0 * a.alpha + (float)r[0]; v1 = v1 * a.alpha + (float)r[1]; v2 = v2 * a.alpha + (float)r[2]; v3 = v3 * a.alpha + (float)r[3];
      }
      if (has2) {
        rd_h4 r = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
        if (in) r = *reinterpret_cast<const rd_h4*>(a.r2 + ((size_t)gy * a.W + gx) * a.r2_stride + ch);
        v0 = v0 * a.beta + (float)r[0]; v1 = v1 * a.beta + (float)r[1]; v2 = v2 * a.beta + (float)r[2]; v3 = v3 * a.beta + (float)r[3];
      }
      const rd_h4 hv = {(_Float16)v0, (_Float16)v1, (_Float16)v2, (_Float16)v3};
      *reinterpret_cast<rd_h4*>(rd_lds + ((row0 + m) * RD_TW + li) * OP + ch * 2) = hv;
    }
  }
  __syncthreads();
  for (int t = tid; t < RD_TW * RD_TH * 4 * NT; t += 256) {
    const int c = t % (4 * NT), pix = t / (4 * NT);
    const int py = pix / RD_TW, px = pix - py * RD_TW;
    const int gy = y0 + py, gx = x0 + px;
    if (gy < a.H && gx < a.W)
      *reinterpret_cast<uint4*>(a.y + ((size_t)gy * a.W + gx) * a.y_stride + a.y_offset + c * 8) = *reinterpret_cast<const uint4*>(rd_lds + pix * OP + c * 16);
  }
}

// The entry point (vd3d_conv3x3_dense_f16) has checked every argument; false: the dynamic-LDS attribute could not be set.
bool vd_launch_conv3x3_dense_f16(hipStream_t s, const void* x, int H, int W, int x_stride, int Cin, const void* wfrag, const float* bias, int Cout,
                                 float slope, float alpha, const void* r1, int r1_stride, float beta, const void* r2, int r2_stride, int up2,
                                 void* y, int y_stride, int y_offset) {
  static bool attr_set[64] = {};
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_conv3x3_dense_f16<1, false>), RD_LDS}, {reinterpret_cast<const void*>(k_conv3x3_dense_f16<2, false>), RD_LDS},
                     {reinterpret_cast<const void*>(k_conv3x3_dense_f16<2, true>), RD_LDS}}, attr_set)) return false;
  rd_args a;
  a.x = (const _Float16*)x; a.H = H; a.W = W; a.x_stride = x_stride; a.nch = Cin / 32;
  a.wfrag = (const uint4*)wfrag; a.bias = bias; a.slope = slope; a.alpha = alpha; a.beta = beta;
  a.r1 = (const _Float16*)r1; a.r1_stride = r1_stride; a.r2 = (const _Float16*)r2; a.r2_stride = r2_stride;
  a.y = (_Float16*)y; a.y_stride = y_stride; a.y_offset = y_offset;
  a.ntx = (W + RD_TW - 1) / RD_TW; a.ntiles = a.ntx * ((H + RD_TH - 1) / RD_TH); a.per = (a.ntiles + 7) / 8;
  const dim3 grid(8 * a.per);
  if (Cout == 32) hipLaunchKernelGGL((k_conv3x3_dense_f16<1, false>), grid, dim3(256), RD_LDS, s, a);
  else if (up2) hipLaunchKernelGGL((k_conv3x3_dense_f16<2, true>), grid, dim3(256), RD_LDS, s, a);
  else hipLaunchKernelGGL((k_conv3x3_dense_f16<2, false>), grid, dim3(256), RD_LDS, s, a);
  return true;
}

// The first 3 channels of an fp16 NHWC [H][W][32] map (conv_last, zero-padded to 32 output channels) -> the float32 planar [3][H][W] prediction
// vd3d_esr_postprocess takes.  One thread per pixel: an 8-byte load, three coalesced float32 row stores.
__global__ __launch_bounds__(256) void k_nhwc_f16_to_planar3(const _Float16* __restrict__ t, long long n, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const rd_h4 hv = *reinterpret_cast<const rd_h4*>(t + i * 32);
  out[i] = (float)hv[0];
  out[n + i] = (float)hv[1];
  out[2 * n + i] = (float)hv[2];
}
void vd_launch_nhwc_f16_to_planar3_f32(hipStream_t s, const void* t, int H, int W, float* out) {
  const long long n = (long long)H * W;
  hipLaunchKernelGGL(k_nhwc_f16_to_planar3, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const _Float16*)t, n, out);
}
