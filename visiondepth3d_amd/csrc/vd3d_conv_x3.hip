// vd3d_conv_x3.hip -- the tile convolution in the bf16x3 arithmetic (vd3d_x3.h): ONE kernel (k_conv_x3, vd3d_conv_x3.h) behind two entry points here,
//   vd3d_conv3x3_x3  the 3 x 3 convolutions of the DPT neck / fusion stage / head (stride 1, zero padding 1, no bias; C_out 32 / 64 / 128 / 256), and
//   vd3d_conv_ifn    the convolutions of the RIFE interpolation network (IFNet HDv3: three IFBlocks of 14; C_out 32 / 64 / 96; bias, per-channel PReLU and
//                    residual in the epilogue, channel slices of strided NHWC buffers).
// and a third one, vd3d_conv3x3_s2_x3 (the reassemble stage's 3 x 3 stride-2 convolution, C_out = 128 n), whose launch is vd3d_conv_s2.hip's and whose weight
// image is packed here.  vd3d_conv3x3_x3's launch takes its checks, argument block and grid from cx_dense_args (vd3d_conv_x3.h), as the other dense launches do;
// vd3d_conv_ifn's strided launch with the epilogue options (cx_launch) fills its own.  The kernel body (cx_conv, vd3d_conv_x3.h) carries a MODE parameter; everything in this file is MODE 0, the fp16x2 form (MODE 1) is
// vd3d_conv_x2t.hip's.
// Arithmetic: every float32 operand is split EXACTLY into three bf16 terms by truncation (x3_split); the products x1 w3, x3 w1, x2 w2, x1 w2, x2 w1 go into a `lo`
// accumulator and x1 w1 into `acc` (v_mfma_f32_32x32x16_bf16, float32 accumulation, small products first), summed in the epilogue; x2 w3, x3 w2, x3 w3 <= 2^-24
// relative are dropped, as in the GEMM.  Float32 NHWC in and out, no weight pre-scaling, no range limit, NaN / Inf in gives NaN out.
//
// The structure is k_conv3x3_x2's (vd3d_conv2.hip), on an LDS plan that fits three terms:
//   implicit GEMM per workgroup, M = 256 pixels = an 8 x 32 tile of the "tile grid" (8 MFMA M tiles = the tile's rows), N = CK output channels, K in steps of 16
//   channels.  512 threads = 8 waves as WM (M) x 8 / WM (N) with NWN N tiles per wave, CK = 32 (8 / WM) NWN: 8 x 1 with 1 (CK 32) or 3 (CK 96) N tiles,
//   4 x 2 (two tile rows per wave) with 1 (CK 64) or 2 (CK 128): 32 / 64 / 96 / 128 accumulator registers x 2.
//   A (pixels): the tile + 1 halo ring (10 x 34 = 340 pixels), ONE 16-channel chunk at a time, fetched ONCE by LDS-DMA into a float32 staging buffer (a chunk
//     ahead; pixels outside the image fetch the zero page), split once into LDS [term 3][k-half 2][pixel 340][8 bf16] (32 640 B, double-buffered); every tap
//     reads its fragments from it: 32 consecutive pixels of a tile row shifted by the tap = consecutive 16-byte slots, conflict-free ds_read_b128.
//   B (weights): packed once per model into the K steps in the order a workgroup runs them, [slice][step][term 3][k-half 2][oc CK][8 bf16] (96 CK bytes per
//     step, a workgroup's steps contiguous), and streamed by LDS-DMA through a ring of four stages, three steps ahead, counted vmcnt + raw s_barrier.  A ring
//     stage is whole 8 KB DMA rounds; the lanes of a round's padding read the zero page (one cache line, no bandwidth).
//   LDS: 2 x 32 640 + 24 576 (staging) + 4 x stage = 122 624 (CK 32, 64: 4 x 8 192), 155 392 (CK 96, 128: 4 x 16 384).
//   Per K step and wave: 3 (8 / WM) A + 3 NWN B ds_read_b128 feed (8 / WM) x NWN x 6 MFMAs.
// Three geometries (template parameter KIND):
//   K3S1  3 x 3, stride 1, padding 1.  Tile grid = output = input.  9 K steps per chunk (tap (dy, dx) = a shift of the fragment address).  C_out 256 runs as
//         two 128-channel slices: one workgroup with all 256 channels would need 2 x 128 accumulator registers for the two-accumulator sum, which two waves per
//         SIMD do not have; each slice fetches and splits the input tile.
//   K3S2  3 x 3, stride 2, padding 1, output (H+1)/2 x (W+1)/2.  The space-to-depth view WITHOUT zero-filled taps: tile grid = output; a staged "chunk" is
//         (16 channels, sub-pixel (sy, sx)) and holds input pixel (2 ty + sy, 2 tx + sx) at tile position (ty, tx).  Output (q, r) reads input rows 2q-1, 2q,
//         2q+1: sub-row 0 serves k_y = 1 at dy = 0, sub-row 1 serves k_y = 0 at dy = -1 and k_y = 2 at dy = 0; the same in x.  So the four sub-pixels run
//         1, 2, 2 and 4 K steps: 9 per 16 channels, no MFMA on zero weights (a zero-weight tap would also carry a NaN to outputs whose window does not hold it).
//         The price is four stagings per 16 channels; this geometry is about 6 % of the interpolation network's MACs.
//   T4S2  ConvTranspose2d(4, stride 2, padding 1), output 2H x 2W, as four output phases, each a 2 x 2 stride-1 convolution of the input: phase p = 0 takes
//         k = 3 at i = q - 1 and k = 1 at i = q, phase p = 1 takes k = 2 at i = q and k = 0 at i = q + 1 (the same in x); output pixel (2q + p_y, 2r + p_x).
//         Tile grid = input.  Each workgroup stages the tile and runs the 4 K steps per chunk of ONE phase.  (All four phases from one staged tile would need
//         4 x the accumulators: 384 registers at 96 output channels.)
// Channels: C_in a multiple of 16 read from pixels of pitch x_stride; C_out written at [y_offset, y_offset + C_out) of pixels of pitch y_stride.
// Epilogue (float32).  vd3d_conv_ifn (EPI): y = acc + lo + bias[oc]; y = y >= 0 ? y : slope[oc] * y (slope == nullptr: none); y += R[pixel][oc] (R == nullptr:
// none).  vd3d_conv3x3_x3: y = acc + lo, nothing else (a bias-free convolution adds no zero either: -0 + 0 is +0).
#include "vd3d_dev.h"
#include "vd3d_conv_x3.h"

#define CX_LDS_MAX 155392                             // the largest dynamic LDS request of any instantiation (CK 96, 128); a workgroup can have 163 840
static_assert(cx_lds(128) == CX_LDS_MAX && cx_lds(96) == CX_LDS_MAX && cx_lds(64) <= CX_LDS_MAX && cx_lds(32) <= CX_LDS_MAX && CX_LDS_MAX <= 163840, "LDS plan");

// ---- weights -> the K-step images [slice][step][term 3][k-half 2][oc CK][8 bf16] in the order a workgroup runs the steps; one thread = (step, k-half, oc): 8
// channels.  K3S1 / K3S2: W[Cout][Cin][3][3]; T4S2: W[Cin][Cout][4][4] (PyTorch's layouts).  CK = Cout, but 128 for a C_out above 128 (K3S1's 256, K3S2's 128 n:
// channel slices, each slice's steps contiguous); the four phases of T4S2 are its slices.
__global__ __launch_bounds__(256) void k_conv_x3_pack(int kind, const float* __restrict__ W, int Cout, int Cin, uint8_t* __restrict__ img) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int nchunk = Cin / 16, spc = kind == CX_T4S2 ? 16 : 9, total = nchunk * spc * 2 * Cout;
  if (t >= total) return;
  const int oc = t % Cout, khf = (t / Cout) & 1, CK = Cout > 128 ? 128 : Cout;
  int step = t / (2 * Cout), c16, ky, kx;
  if (kind == CX_K3S1) { c16 = step / 9; const int tap = step - c16 * 9; ky = tap / 3; kx = tap - ky * 3; step += (oc / CK) * nchunk * 9; }
  else if (kind == CX_K3S2) {   // per 16 channels: sub-pixel (0,0) 1 step, (0,1) 2, (1,0) 2, (1,1) 4
    c16 = step / 9;
    const int j = step - c16 * 9;
    const int sub = j == 0 ? 0 : j < 3 ? 1 : j < 5 ? 2 : 3, tap = j == 0 ? 0 : j < 3 ? j - 1 : j < 5 ? j - 3 : j - 5;
    const int sy = sub >> 1, sx = sub & 1, ty = sx ? tap >> 1 : tap, tx = sx ? tap & 1 : 0;
    ky = sy ? 2 * ty : 1; kx = sx ? 2 * tx : 1;
    step += (oc / CK) * nchunk * 9;
  } else {                      // [phase 4][chunk][tap 4]
    const int phase = step / (nchunk * 4), rem = step - phase * (nchunk * 4);
    c16 = rem >> 2;
    const int tap = rem & 3;
    ky = 3 - (phase >> 1) - 2 * (tap >> 1); kx = 3 - (phase & 1) - 2 * (tap & 1);
  }
  float w[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ci = c16 * 16 + khf * 8 + e;
    w[e] = kind == CX_T4S2 ? W[(((size_t)ci * Cout + oc) * 4 + ky) * 4 + kx] : W[(((size_t)oc * Cin + ci) * 3 + ky) * 3 + kx];
  }
  x3_s8 o[3];
  x3_split8(w, o);
  uint8_t* base = img + (size_t)step * CK * 96 + (khf * CK + oc % CK) * 16;
#pragma unroll
  for (int t3 = 0; t3 < 3; ++t3) *reinterpret_cast<uint4*>(base + t3 * 2 * CK * 16) = __builtin_bit_cast(uint4, o[t3]);
}

// kind, C_in and C_out have been checked by the caller's *_weight_bytes
static long long cx_weight_bytes(int kind, int Cin, int Cout) {
  return (long long)(Cin / 16) * (kind == CX_T4S2 ? 16 : 9) * Cout * 96 + 64;   // step images, 64 zero bytes (the zero page of the padding)
}
static bool cx_pack(hipStream_t s, int kind, const float* W, int Cin, int Cout, void* img) {
  if (reinterpret_cast<uintptr_t>(img) & 15) return false;
  if (hipMemsetAsync(reinterpret_cast<uint8_t*>(img) + cx_weight_bytes(kind, Cin, Cout) - 64, 0, 64, s) != hipSuccess) return false;
  const int total = (Cin / 16) * (kind == CX_T4S2 ? 16 : 9) * 2 * Cout;
  hipLaunchKernelGGL(k_conv_x3_pack, dim3((total + 255) / 256), dim3(256), 0, s, kind, W, Cout, Cin, reinterpret_cast<uint8_t*>(img));
  return true;
}

template <int KIND>
static void cx_launch_kind(hipStream_t s, dim3 grid, int Cout, const vd_cx_args& a) {
  if (Cout == 32) hipLaunchKernelGGL((k_conv_x3<KIND, 8, 1, true>), grid, dim3(CX_NT), cx_lds(32), s, a);
  else if (Cout == 64) hipLaunchKernelGGL((k_conv_x3<KIND, 4, 1, true>), grid, dim3(CX_NT), cx_lds(64), s, a);
  else hipLaunchKernelGGL((k_conv_x3<KIND, 8, 3, true>), grid, dim3(CX_NT), cx_lds(96), s, a);
}
static void cx_launch_plain(hipStream_t s, dim3 grid, int Cout, const vd_cx_args& a) {   // grid: cx_dense_args's, with C_out's 128-channel slices on z
  if (Cout == 32) hipLaunchKernelGGL((k_conv_x3<CX_K3S1, 8, 1, false>), grid, dim3(CX_NT), cx_lds(32), s, a);   // the head's 64 -> 32
  else if (Cout == 64) hipLaunchKernelGGL((k_conv_x3<CX_K3S1, 4, 1, false>), grid, dim3(CX_NT), cx_lds(64), s, a);
  else hipLaunchKernelGGL((k_conv_x3<CX_K3S1, 4, 2, false>), grid, dim3(CX_NT), cx_lds(128), s, a);   // 128, or 256 as two slices
}
// the strided launch with the epilogue options (vd3d_conv_ifn).  false: the dynamic-LDS attribute could not be set
static bool cx_launch(hipStream_t s, int kind, const float* X, int B, int H, int W, int x_stride, int Cin, const void* wimg, const float* bias, const float* slope,
                      int Cout, const float* R, int r_stride, float* Y, int y_stride, int y_offset) {
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
#define CX_FN(K) {reinterpret_cast<const void*>(k_conv_x3<K, 8, 1, true>), cx_lds(32)}, {reinterpret_cast<const void*>(k_conv_x3<K, 4, 1, true>), cx_lds(64)}, \
                 {reinterpret_cast<const void*>(k_conv_x3<K, 8, 3, true>), cx_lds(96)}
  if (!vd_lds_optin({CX_FN(CX_K3S1), CX_FN(CX_K3S2), CX_FN(CX_T4S2)}, attr_set)) return false;
#undef CX_FN
  vd_cx_args a;
  const uint8_t* wi = reinterpret_cast<const uint8_t*>(wimg);
  a.X = X; a.Wimg = wi; a.zero16 = reinterpret_cast<const float*>(wi + cx_weight_bytes(kind, Cin, Cout) - 64); a.bias = bias; a.slope = slope; a.R = R; a.Y = Y;
  a.B = B; a.H = H; a.W = W;
  a.Ho = kind == CX_K3S2 ? (H + 1) / 2 : kind == CX_T4S2 ? 2 * H : H;
  a.Wo = kind == CX_K3S2 ? (W + 1) / 2 : kind == CX_T4S2 ? 2 * W : W;
  a.x_stride = x_stride; a.y_stride = y_stride; a.y_offset = y_offset; a.r_stride = r_stride; a.nchunk = Cin / 16; a.colscale = nullptr;
  a.R2 = nullptr; a.Y2 = nullptr; a.relu_in = 0; a.relu = 0; a.b3 = 0.f;
  const int gh = kind == CX_K3S2 ? a.Ho : H, gw = kind == CX_K3S2 ? a.Wo : W;   // the tile grid
  a.ntx = (gw + CX_TW - 1) / CX_TW;
  const dim3 grid((unsigned)(a.ntx * ((gh + CX_TH - 1) / CX_TH)), (unsigned)B, kind == CX_T4S2 ? 4u : 1u);
  if (kind == CX_K3S1) cx_launch_kind<CX_K3S1>(s, grid, Cout, a);
  else if (kind == CX_K3S2) cx_launch_kind<CX_K3S2>(s, grid, Cout, a);
  else cx_launch_kind<CX_T4S2>(s, grid, Cout, a);
  return true;
}

// ---- vd3d_conv3x3_x3: K3S1 on dense maps (pitches C_in and C_out), no bias, slope or residual
long long vd_conv3x3_x3_weight_bytes(int Cin, int Cout) {
  if (Cin < 16 || (Cin & 15) || (Cout != 32 && Cout != 64 && Cout != 128 && Cout != 256)) return -1;
  return cx_weight_bytes(CX_K3S1, Cin, Cout);
}
bool vd_launch_conv3x3_x3_pack(hipStream_t s, const float* W, int Cin, int Cout, void* img) {
  return vd_conv3x3_x3_weight_bytes(Cin, Cout) >= 0 && cx_pack(s, CX_K3S1, W, Cin, Cout, img);
}
bool vd_launch_conv3x3_x3(hipStream_t s, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, float* Y) {
  const long long wb = vd_conv3x3_x3_weight_bytes(Cin, Cout);
  vd_cx_args a;
  dim3 grid;
  if (wb < 0 || !cx_dense_args(CX_K3S1, X, B, H, W, Cin, wimg, Cout, Y, nullptr, reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(wimg) + wb - 64), a, grid))
    return false;
  static bool attr_set[64] = {};   // per device, as in cx_launch
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_conv_x3<CX_K3S1, 8, 1, false>), cx_lds(32)}, {reinterpret_cast<const void*>(k_conv_x3<CX_K3S1, 4, 1, false>), cx_lds(64)},
                     {reinterpret_cast<const void*>(k_conv_x3<CX_K3S1, 4, 2, false>), cx_lds(128)}}, attr_set)) return false;
  cx_launch_plain(s, grid, Cout, a);
  return true;
}

// ---- vd3d_conv3x3_s2_x3 (host half; the launch is vd3d_conv_s2.hip's): K3S2 on dense maps, C_out = 128 n as n channel slices
long long vd_conv3x3_s2_x3_weight_bytes(int Cin, int Cout) {
  if (Cin < 16 || (Cin & 15) || Cin > 65536 || Cout < 128 || (Cout & 127) || Cout > 1024) return -1;
  return cx_weight_bytes(CX_K3S2, Cin, Cout);
}
bool vd_launch_conv3x3_s2_x3_pack(hipStream_t s, const float* W, int Cin, int Cout, void* img) {
  return vd_conv3x3_s2_x3_weight_bytes(Cin, Cout) >= 0 && cx_pack(s, CX_K3S2, W, Cin, Cout, img);
}

// ---- vd3d_conv_ifn: the entry point has checked every argument
long long vd_conv_ifn_weight_bytes(int kind, int Cin, int Cout) {
  if (kind < CX_K3S1 || kind > CX_T4S2 || Cin < 16 || (Cin & 15) || Cin > 65536 || (Cout != 32 && Cout != 64 && Cout != 96)) return -1;
  return cx_weight_bytes(kind, Cin, Cout);
}
bool vd_launch_conv_ifn_pack(hipStream_t s, int kind, const float* W, int Cin, int Cout, void* img) {
  return vd_conv_ifn_weight_bytes(kind, Cin, Cout) >= 0 && cx_pack(s, kind, W, Cin, Cout, img);
}
bool vd_launch_conv_ifn(hipStream_t s, int kind, const float* X, int B, int H, int W, int x_stride, int Cin, const void* wimg, const float* bias,
                        const float* slope, int Cout, const float* R, int r_stride, float* Y, int y_stride, int y_offset) {
  if (vd_conv_ifn_weight_bytes(kind, Cin, Cout) < 0 || B < 1 || B > 65535 || H < 1 || W < 1) return false;
  return cx_launch(s, kind, X, B, H, W, x_stride, Cin, wimg, bias, slope, Cout, R, r_stride, Y, y_stride, y_offset);
}
