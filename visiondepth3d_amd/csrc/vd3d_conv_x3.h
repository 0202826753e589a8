// vd3d_conv_x3.h -- the tile-convolution kernel of vd3d_conv_x3.hip (its header comment describes the plan): the LDS layout constants, the argument block and
// the kernel body cx_conv<MODE, ...>, shared by the translation units that instantiate it: vd3d_conv_x3.hip (vd3d_conv3x3_x3, vd3d_conv_ifn) and vd3d_conv_s2.hip
// (vd3d_conv3x3_s2_x3) as k_conv_x3 = MODE 0 (bf16x3), vd3d_conv_x2t.hip (vd3d_conv3x3_s1_x2, vd3d_conv3x3_s2_x2) as k_conv_x2 = MODE 1 (fp16x2, vd3d_x3.h).
// MODE 1 differs in four places and nowhere else: two operand terms instead of three (a chunk image of 2 x 2 planes = 21 760 bytes, a K step of 64 CK bytes:
// one DMA round per stage for every CK), the round-to-nearest fp16 split of the staged pixels, three products per K step (x1 w2, x2 w1 into `lo`, x1 w1 into `acc`;
// x2 w2 dropped) on v_mfma_f32_32x32x16_f16, and an epilogue that multiplies acc + lo by colscale[oc], the exact power of two the packer divided the channel's
// weights by.  The DMA counts behind the counted waits are NBP and CX_A_ITERS in both modes (the staging buffer is float32 either way).
// At the end, host side: cx_dense_args, the checks, argument block and grid of the four dense, bias-free entry points; their launchers keep the kernel selection.
#pragma once
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include "vd3d_x3.h"

#define CX_TH 8
#define CX_TW 32
#define CX_PH (CX_TH + 2)
#define CX_PW (CX_TW + 2)
#define CX_NPIX (CX_PH * CX_PW)                       // 340
#define CX_NT 512
#define CX_NS 4                                       // weight ring stages
#define CX_PLANE (CX_NPIX * 16)                       // one (term, k-half) plane: 5 440 bytes
#define CX_A_BUF (3 * 2 * CX_PLANE)                   // one chunk image: 32 640 bytes
#define CX_A_ITEMS (CX_NPIX * 4)                      // (pixel, 4-channel quad) items of a chunk: 1 360
#define CX_A_ITERS ((CX_A_ITEMS + CX_NT - 1) / CX_NT) // 3 per thread
#define CX_A_STG (CX_A_ITERS * CX_NT * 16)            // float32 staging buffer of one chunk, item-linear (what a DMA instruction can write): 24 576 bytes
__host__ __device__ constexpr int cx_b_stage(int ck) { return (3 * 2 * ck * 16 + 8191) / 8192 * 8192; }   // 8 192 (32, 64), 16 384 (96, 128)
#define CX_B_OFF (2 * CX_A_BUF + CX_A_STG)
__host__ __device__ constexpr int cx_lds(int ck) { return CX_B_OFF + CX_NS * cx_b_stage(ck); }
// the same plan by MODE (0: the numbers above)
__host__ __device__ constexpr int cx_terms(int mode) { return mode == 0 ? 3 : 2; }
__host__ __device__ constexpr int cx_a_buf(int mode) { return cx_terms(mode) * 2 * CX_PLANE; }                // 32 640 | 21 760
__host__ __device__ constexpr int cx_b_step(int mode, int ck) { return cx_terms(mode) * 2 * ck * 16; }       // 96 CK | 64 CK bytes
__host__ __device__ constexpr int cx_b_stage_m(int mode, int ck) { return (cx_b_step(mode, ck) + 8191) / 8192 * 8192; }   // MODE 1: 8 192 for every CK
__host__ __device__ constexpr int cx_b_off(int mode) { return 2 * cx_a_buf(mode) + CX_A_STG; }               // 89 856 | 68 096
__host__ __device__ constexpr int cx_lds_m(int mode, int ck) { return cx_b_off(mode) + CX_NS * cx_b_stage_m(mode, ck); }   // MODE 1: 100 864
static_assert(cx_a_buf(0) == CX_A_BUF && cx_b_off(0) == CX_B_OFF && cx_lds_m(0, 128) == cx_lds(128) && cx_lds_m(0, 32) == cx_lds(32), "MODE 0 is the plan above");

enum { CX_K3S1 = 0, CX_K3S2 = 1, CX_T4S2 = 2 };   // include/vd3d.h VD3D_IFN_*
VD_DEV float cx_relu_nan(float x) { return x != x ? x : fmaxf(x, 0.f); }   // torch.relu: a NaN stays a NaN (fmaxf alone would give 0)

struct vd_cx_args {
  const float* X; const uint8_t* Wimg; const float* zero16; const float* bias; const float* slope; const float* R; float* Y;
  int B, H, W;              // the input map
  int Ho, Wo;               // the output map
  int x_stride, y_stride, y_offset, r_stride;
  int ntx;                  // tiles per row of the tile grid
  int nchunk;               // C_in / 16
  const float* colscale;    // MODE 1: 2^-e per output channel (the weight image holds 2^e W); MODE 0: not read
  // EPI 2 only (vd3d_conv3x3_epi; behind everything the other forms read, so their argument offsets are what they were)
  const float* R2; float* Y2; int relu_in, relu;
  float b3;                 // EPI 3 only (vd3d_depthpro_head): the bias of the 1 x 1 convolution to one channel
};

// EPI: the entry points' thin variants of the one body.  1 / true (vd3d_conv_ifn): + bias (never null there), optional slope and residual, at most 96 output
// channels.  0 / false (vd3d_conv3x3_x3: K3S1; vd3d_conv3x3_s2_x3: K3S2): the bare sum -- nothing is added, not even a zero -- and CK-channel slices of C_out on
// the grid's z axis (K3S1: 256 as two slices of 128; K3S2: 128 n as n slices).  2 (vd3d_conv3x3_epi, vd3d_conv_epi.hip: K3S1, both MODEs): the bare sum of
// EPI 0, sliced the same way, over X or over relu(X) (relu_in: applied to the staged pixels in front of the split, a NaN stays a NaN), then
// vd3d_nhwc_bias_act_f32's chain on the sum in registers: [+ bias[oc]] [+ R] [R2 + v] [max(v, 0)] -> Y, [max(v, 0) -> Y2]; every operand but X is optional.
// 3 (vd3d_depthpro_head, vd3d_depthpro_head.hip: T4S2 with 32 output channels, both MODEs): the whole tail of DepthPro's head behind the sum -- a border-class
// bias table, ReLU, the 1 x 1 convolution to ONE channel as a butterfly over the 32 lanes of a pixel, its bias, ReLU -- one float per output pixel.
template <int MODE, int KIND, int WM, int NWN, int EPI>
VD_DEV void cx_conv(const vd_cx_args a) {
  constexpr int NTM = cx_terms(MODE), A_BUF = cx_a_buf(MODE), B_OFF = cx_b_off(MODE);
  constexpr int NS = CX_NS, WN = 8 / WM, MR = CX_TH / WM, CK = 32 * WN * NWN, BST = cx_b_stage_m(MODE, CK), NBP = BST / (CX_NT * 16), B_ITEMS = 2 * NTM * CK;
  static_assert(MODE == 0 || EPI != 1, "the fp16x2 form has no interpolation-network epilogue");
  static_assert(EPI != 2 || KIND == CX_K3S1, "the residual-unit epilogue is built for the stride-1 geometry");
  constexpr int A_FLY = NS - 2;   // the taps of a chunk whose counted wait leaves the next chunk's pixel DMAs in flight
  constexpr int SUBS = KIND == CX_K3S2 ? 4 : 1, ST = KIND == CX_K3S2 ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) uint8_t cx_smem[];   // the only LDS object: [A buffer 0][A buffer 1][float32 staging][B ring]
  const int tile = blockIdx.x, b = blockIdx.y;
  // blockIdx.z is the weight slice of the workgroup: the output phase 2 p_y + p_x for T4S2, the CK-channel slice of C_out without EPI (K3S1: 0 or 1, C_out
  // 256; K3S2: C_out / 128 slices); otherwise the grid has one z plane and it is not read
  constexpr bool SLICED = KIND == CX_T4S2 || EPI != 1;
  const unsigned slice = SLICED ? blockIdx.z : 0u;
  const int ph_y = KIND == CX_T4S2 ? (int)(slice >> 1) : 0, ph_x = KIND == CX_T4S2 ? (int)(slice & 1) : 0, oc0 = KIND == CX_T4S2 ? 0 : (int)slice * CK;
  const int tyi = tile / a.ntx, txi = tile - tyi * a.ntx;
  const int y0 = tyi * CX_TH, x0 = txi * CX_TW;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - wm * WN, li = lane & 31, kh = lane >> 5;
  const int wave_base = (tid & ~63) * 16;

  // ---- A staging: item i = it * 512 + tid -> (pixel = i >> 2 of the 10 x 34 halo tile, quad = i & 3 = four of the chunk's 16 channels); the DMA of item i lands
  // in staging slot i.  A pixel outside the image (zero padding) or an item past the tile fetches the 64 zero bytes behind the weight image.
  int aty[CX_A_ITERS], atx[CX_A_ITERS], adst[CX_A_ITERS];
  const int q4 = tid & 3;
#pragma unroll
  for (int it = 0; it < CX_A_ITERS; ++it) {
    const int i = it * CX_NT + tid, pix = i >> 2;
    const int py = pix / CX_PW, px = pix - py * CX_PW;
    aty[it] = i < CX_A_ITEMS ? y0 - 1 + py : -(1 << 28);   // an item past the tile is "above the image"
    atx[it] = x0 - 1 + px;
    adst[it] = i < CX_A_ITEMS ? ((q4 >> 1) * CX_NPIX + pix) * 16 + (q4 & 1) * 8 : -1;   // + term * 2 * CX_PLANE
  }
  const float* xb = a.X + (size_t)b * a.H * a.W * a.x_stride + q4 * 4;
  auto load_a = [&](int chunk) {   // chunk = c16 * SUBS + (sy * 2 + sx)
    const int c16 = chunk / SUBS, sy = KIND == CX_K3S2 ? (chunk >> 1) & 1 : 0, sx = KIND == CX_K3S2 ? chunk & 1 : 0;
#pragma unroll
    for (int it = 0; it < CX_A_ITERS; ++it) {
      const int gy = ST * aty[it] + sy, gx = ST * atx[it] + sx;
      const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      const float* p = in ? xb + ((size_t)gy * a.W + gx) * a.x_stride + c16 * 16 : a.zero16;
      __builtin_amdgcn_global_load_lds((x3_glb_vp)p, (x3_lds_vp)(cx_smem + 2 * A_BUF + it * (CX_NT * 16) + wave_base), 16, 0, 0);
    }
  };
  auto write_a = [&](int buf) {   // staging (float32) -> exact three-term split (MODE 1: round-to-nearest two-term split) -> one 8-byte LDS store per term and item
    uint8_t* dst = cx_smem + buf * A_BUF;
    const uint8_t* stg = cx_smem + 2 * A_BUF + tid * 16;
#pragma unroll
    for (int it = 0; it < CX_A_ITERS; ++it) {
      const x3_s8 raw = *reinterpret_cast<const x3_s8*>(stg + it * (CX_NT * 16));   // a short vector, bit-cast: not ordered behind the DMAs in flight (vd3d_x3.h)
      float4 f = __builtin_bit_cast(float4, raw);
      if constexpr (EPI == 2) {
        if (a.relu_in) { f.x = cx_relu_nan(f.x); f.y = cx_relu_nan(f.y); f.z = cx_relu_nan(f.z); f.w = cx_relu_nan(f.w); }   // uniform
      }
      if constexpr (MODE == 1) {
        const float v[4] = {f.x, f.y, f.z, f.w};
        x3_h4 h1, h2;
        x3_split4_h(v, h1, h2);
        if (adst[it] >= 0) {
          *reinterpret_cast<x3_h4*>(dst + adst[it]) = h1;
          *reinterpret_cast<x3_h4*>(dst + 2 * CX_PLANE + adst[it]) = h2;
        }
      } else {
        uint32_t t1[4], t2[4], t3[4];
        x3_split(f.x, t1[0], t2[0], t3[0]); x3_split(f.y, t1[1], t2[1], t3[1]); x3_split(f.z, t1[2], t2[2], t3[2]); x3_split(f.w, t1[3], t2[3], t3[3]);
        if (adst[it] >= 0) {
          *reinterpret_cast<x3_u2*>(dst + adst[it]) = x3_u2{x3_pack(t1[0], t1[1]), x3_pack(t1[2], t1[3])};
          *reinterpret_cast<x3_u2*>(dst + 2 * CX_PLANE + adst[it]) = x3_u2{x3_pack(t2[0], t2[1]), x3_pack(t2[2], t2[3])};
          *reinterpret_cast<x3_u2*>(dst + 4 * CX_PLANE + adst[it]) = x3_u2{x3_pack(t3[0], t3[1]), x3_pack(t3[2], t3[3])};
        }
      }
    }
  };
  // ---- B staging: the slice's K steps are contiguous in the packed image, [step][term NTM][k-half 2][oc CK][8 bf16 | fp16]; item i = p * 512 + tid is 16 bytes
  // of a step; the items behind the step's 96 CK (MODE 1: 64 CK) bytes read the zero page
  const int NCH = a.nchunk * SUBS;
  const int KS = KIND == CX_T4S2 ? a.nchunk * 4 : a.nchunk * 9;
  const size_t bstep = (size_t)cx_b_step(MODE, CK);
  const uint8_t* wbase = a.Wimg + (SLICED ? (size_t)slice * KS * bstep : (size_t)0);
  auto stage_b = [&](int ks, int slot) {
#pragma unroll
    for (int p = 0; p < NBP; ++p) {
      const int i = p * CX_NT + tid;
      const uint8_t* src = i < B_ITEMS ? wbase + (size_t)ks * bstep + i * 16 : reinterpret_cast<const uint8_t*>(a.zero16);
      __builtin_amdgcn_global_load_lds((x3_glb_vp)src, (x3_lds_vp)(cx_smem + B_OFF + slot * BST + p * (CX_NT * 16) + wave_base), 16, 0, 0);
    }
  };

  // Two accumulators per tile: x1 w1 in `acc`, the five correction products (<= 2^-7 of it) in `lo`, summed in the epilogue.  One float32 rounding at the
  // running sum's magnitude per K step instead of six: with a single accumulator the 1024-channel neck convolution (55 296 MFMA adds per output) measured a
  // relative RMS error 1.8 x that of a float32 CPU convolution, outside the bar of tests/test_hip_conv_x3.py.
  x3_f16 acc[MR][NWN], lo[MR][NWN];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NWN; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = lo[m][n][r] = 0.f;

  load_a(0);
#pragma unroll
  for (int st = 0; st < NS - 1; ++st) stage_b(st < KS ? st : KS - 1, st);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prologue waits for everything; a thread converts only the staging slots its OWN DMA lanes filled
  write_a(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // fragment base offsets: A: k-half plane, tile row MR wm + m (+ 1 halo + dy), column li (+ 1 + dx); B: k-half plane, output channel (wn * NWN + n) * 32 + li
  const int fa_base = (kh * CX_NPIX + (MR * wm + 1) * CX_PW + li + 1) * 16;
  const int fb_base = B_OFF + (kh * CK + wn * NWN * 32 + li) * 16;
  int ks = 0;
  for (int chunk = 0; chunk < NCH; ++chunk) {
    const bool more_a = chunk + 1 < NCH;   // uniform
    if (more_a) load_a(chunk + 1);
    const uint8_t* sa = cx_smem + (chunk & 1) * A_BUF;
    const int sy = KIND == CX_K3S2 ? (chunk >> 1) & 1 : 0, sx = KIND == CX_K3S2 ? chunk & 1 : 0;
    const int T = KIND == CX_K3S1 ? 9 : KIND == CX_T4S2 ? 4 : (1 + sy) * (1 + sx);
#pragma unroll 1
    for (int tap = 0; tap < T; ++tap, ++ks) {
      int dy, dx;
      if (KIND == CX_K3S1) { dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
      else if (KIND == CX_T4S2) { dy = ph_y + (tap >> 1) - 1; dx = ph_x + (tap & 1) - 1; }
      else { const int ty = sx ? tap >> 1 : tap, tx = sx ? tap & 1 : 0; dy = ty - sy; dx = tx - sx; }
      const int slot = ks % NS;
      stage_b(ks + NS - 1 < KS ? ks + NS - 1 : KS - 1, (ks + NS - 1) % NS);   // behind the last step: a harmless re-fetch (straight-line code, one counted wait)
      const uint8_t* sb = cx_smem + slot * BST;
      const uint8_t* sat = sa + fa_base + (dy * CX_PW + dx) * 16;
      x3_s8 af[MR][NTM];
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int t = 0; t < NTM; ++t) af[m][t] = *reinterpret_cast<const x3_s8*>(sat + t * (2 * CX_PLANE) + m * (CX_PW * 16));
#pragma unroll
      for (int n = 0; n < NWN; ++n) {
        x3_s8 bf[NTM];
#pragma unroll
        for (int t = 0; t < NTM; ++t) bf[t] = *reinterpret_cast<const x3_s8*>(sb + fb_base + t * (2 * CK * 16) + n * 512);
        // small products first, into their own accumulator; the M tiles alternate so that dependent MFMAs are not back to back
#define CX_MM(ACC, ta, tb) _Pragma("unroll") for (int m = 0; m < MR; ++m) ACC[m][n] = x3_mfma<MODE>(af[m][ta], bf[tb], ACC[m][n]);
        if constexpr (MODE == 0) { CX_MM(lo, 0, 2) CX_MM(lo, 2, 0) CX_MM(lo, 1, 1) CX_MM(lo, 0, 1) CX_MM(lo, 1, 0) CX_MM(acc, 0, 0) }
        else { CX_MM(lo, 0, 1) CX_MM(lo, 1, 0) CX_MM(acc, 0, 0) }   // x1 w2, x2 w1; x1 w1
#undef CX_MM
      }
      // Counted wait.  In flight, oldest first: B (ks + 1) .. B (ks + NS - 1), with the next chunk's CX_A_ITERS pixel DMAs issued in front of this chunk's tap 0
      // B round.  The next step needs B (ks + 1): while fewer than NS - 1 B rounds have followed the pixel DMAs (tap < NS - 2) they are younger than B (ks + 1)
      // and stay in flight with the NS - 2 younger B rounds; from tap NS - 2 on they are older than what must land, so they land too.
      if (more_a && tap < A_FLY) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * NBP + CX_A_ITERS) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * NBP) : "memory");
      // Split the next chunk's pixels into the other buffer (last read in the previous chunk).  They have landed at tap NS - 2's wait, so tap NS - 1 is the first
      // step that can do it, and the DPT stride-1 convolution does it there; the interpolation network's geometries have chunks shorter than that (K3S2) and do
      // it at the chunk's last step, all three alike, and so does K3S2 without EPI (its 1- and 2-step chunks never reach tap NS - 1).  Either position is safe;
      // each entry point keeps the one it was measured with.
      if (more_a && tap == (EPI == 1 || KIND == CX_K3S2 ? T : NS) - 1) {
        if (KIND == CX_K3S2 && T < NS - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a 1- or 2-step chunk: the pixel DMAs have not been waited for yet
        write_a((chunk + 1) & 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  if constexpr (EPI == 3) {
    // ---- the DepthPro head's epilogue (vd3d_depthpro_head.hip; T4S2, 8 x 1 waves, CK = 32: a wave owns one tile row, lane (li, kh) holds output channel li of
    // the 16 columns (r & 3) + 8 (r >> 2) + 4 kh).  Per pixel: u = max(v + T[row class][column class][oc], 0), d = sum over oc of w3[oc] u as a butterfly over
    // the 32 lanes of the pixel (partner distance 16, 8, 4, 2, 1, in that order: every lane ends with the same bits), out = max(d + b3, 0); lane li < 16
    // stores the pixel of register li.  All 64 lanes run the butterflies; only the store is masked.  a.bias = T [3][3][32], a.slope = w3 [32].
    static_assert(KIND == CX_T4S2 && WM == 8 && NWN == 1, "the head epilogue reduces the 32 channels of one N tile");
    const int oy = 2 * (y0 + wm) + ph_y;
    const int ry = oy == 0 ? 0 : oy == a.Ho - 1 ? 2 : 1;   // first / interior / last fine row (a row past the map reads the interior class and stores nothing)
    const float t0 = a.bias[(ry * 3 + 0) * 32 + li], t1 = a.bias[(ry * 3 + 1) * 32 + li], t2 = a.bias[(ry * 3 + 2) * 32 + li], w3 = a.slope[li];
    float cs = 1.f;
    if constexpr (MODE == 1) cs = a.colscale[li];
    float mine = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ox = 2 * (x0 + (r & 3) + 8 * (r >> 2) + 4 * kh) + ph_x;
      float v = acc[0][0][r] + lo[0][0][r];
      if constexpr (MODE == 1) v *= cs;
      float d = w3 * fmaxf(v + (ox == 0 ? t0 : ox == a.Wo - 1 ? t2 : t1), 0.f);
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) d = d + __shfl_xor(d, off, 64);
      if (li == r) mine = d;
    }
    const int ox = 2 * (x0 + (li & 3) + 8 * ((li & 15) >> 2) + 4 * kh) + ph_x;
    if (li < 16 && oy < a.Ho && ox < a.Wo) a.Y[((size_t)b * a.Ho + oy) * a.Wo + ox] = fmaxf(mine + a.b3, 0.f);
    return;
  }

  // ---- epilogue: accumulator register r of (m, n) = tile column (r & 3) + 8 (r >> 2) + 4 kh of tile row MR wm + m, output channel oc0 + (wn * NWN + n) * 32 + li
#pragma unroll
  for (int n = 0; n < NWN; ++n) {
    const int oc = oc0 + (wn * NWN + n) * 32 + li;
    float bv = 0.f, sv = 1.f;
    if constexpr (EPI == 1) { bv = a.bias[oc]; sv = a.slope ? a.slope[oc] : 1.f; }
    if constexpr (EPI == 2) { if (a.bias) bv = a.bias[oc]; }
    float cs = 1.f;
    if constexpr (MODE == 1) { cs = a.colscale[oc]; asm volatile("" : "+v"(cs)); }   // consumed in front of the masked stores (vd3d_gemm.hip: else one s_waitcnt vmcnt(0) per store)
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int ty = y0 + MR * wm + m;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tx = x0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int oy = KIND == CX_T4S2 ? 2 * ty + ph_y : ty, ox = KIND == CX_T4S2 ? 2 * tx + ph_x : tx;
        if (oy < a.Ho && ox < a.Wo) {
          const size_t pix = ((size_t)b * a.Ho + oy) * a.Wo + ox;
          float v = acc[m][n][r] + lo[m][n][r];
          if constexpr (MODE == 1) v *= cs;
          if constexpr (EPI == 1) {
            v += bv;
            if (a.slope) v = v >= 0.f ? v : sv * v;
            if (a.R) v += a.R[pix * a.r_stride + oc];
          }
          if constexpr (EPI == 2) {   // k_bias_act's chain (vd3d_netops.hip), operation for operation
            if (a.bias) v += bv;
            if (a.R) v += a.R[pix * a.r_stride + oc];
            if (a.R2) v = a.R2[pix * a.r_stride + oc] + v;
            if (a.relu) v = fmaxf(v, 0.f);
            if (a.Y2) a.Y2[pix * a.y_stride + oc] = fmaxf(v, 0.f);
          }
          a.Y[pix * a.y_stride + a.y_offset + oc] = v;
        }
      }
    }
  }
}

// the bf16x3 kernel of vd3d_conv_x3.hip / vd3d_conv_s2.hip / vd3d_conv_ifn.hip and the fp16x2 kernel of vd3d_conv_x2t.hip
template <int KIND, int WM, int NWN, bool EPI>
__global__ __launch_bounds__(CX_NT) void k_conv_x3(const vd_cx_args a) { cx_conv<0, KIND, WM, NWN, EPI ? 1 : 0>(a); }
template <int KIND, int WM, int NWN>
__global__ __launch_bounds__(CX_NT) void k_conv_x2(const vd_cx_args a) { cx_conv<1, KIND, WM, NWN, 0>(a); }
// the residual-unit form of either arithmetic (vd3d_conv_epi.hip): stride 1, EPI 2
template <int MODE, int WM, int NWN>
__global__ __launch_bounds__(CX_NT) void k_conv_epi(const vd_cx_args a) { cx_conv<MODE, CX_K3S1, WM, NWN, 2>(a); }
// DepthPro's head behind head.layers.0 in either arithmetic (vd3d_depthpro_head.hip): T4S2, 32 output channels, EPI 3
template <int MODE>
__global__ __launch_bounds__(CX_NT) void k_depthpro_head(const vd_cx_args a) { cx_conv<MODE, CX_T4S2, 8, 1, 3>(a); }

// ---- host: the dense, bias-free launch that vd3d_conv3x3_x3, vd3d_conv3x3_s2_x3, vd3d_conv3x3_s1_x2 and vd3d_conv3x3_s2_x2 share (kind K3S1 or K3S2; the tile
// grid is the output in both).  Checks what they all check -- B 1 .. 65535 (one grid row per frame), a map of at least 1 x 1, X and the image 16-byte and Y
// 4-byte aligned -- and fills the argument block for maps of pitch C_in / C_out and the grid: tiles x frames x 128-channel slices of C_out (one slice below 128).
// zero16: the image's zero page; colscale: MODE 1's, nullptr in MODE 0.  The caller has checked C_in and C_out and keeps its kernel selection and LDS opt-in.
inline bool cx_dense_args(int kind, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, float* Y, const float* colscale, const float* zero16,
                          vd_cx_args& a, dim3& grid) {
  if (B < 1 || H < 1 || W < 1 || B > 65535) return false;
  if ((reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(wimg) & 15) || (reinterpret_cast<uintptr_t>(Y) & 3)) return false;
  a.X = X; a.Wimg = reinterpret_cast<const uint8_t*>(wimg); a.zero16 = zero16; a.bias = nullptr; a.slope = nullptr; a.R = nullptr; a.Y = Y;
  a.B = B; a.H = H; a.W = W;
  a.Ho = kind == CX_K3S2 ? (H + 1) / 2 : H; a.Wo = kind == CX_K3S2 ? (W + 1) / 2 : W;
  a.x_stride = Cin; a.y_stride = Cout; a.y_offset = 0; a.r_stride = 0; a.nchunk = Cin / 16; a.colscale = colscale;
  a.R2 = nullptr; a.Y2 = nullptr; a.relu_in = 0; a.relu = 0; a.b3 = 0.f;
  a.ntx = (a.Wo + CX_TW - 1) / CX_TW;
  grid = dim3((unsigned)(a.ntx * ((a.Ho + CX_TH - 1) / CX_TH)), (unsigned)B, Cout > 128 ? (unsigned)(Cout / 128) : 1u);
  return true;
}
