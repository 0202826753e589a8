// vd3d_conv3.hip -- the 3 x 3 convolutions of the DPT neck / fusion stage / head (stride 1, zero padding 1, no bias, groups 1) in the bf16x3 arithmetic of
// vd3d_gemm.hip: every float32 operand split EXACTLY into three bf16 terms by truncation (gx_split: 8 + 8 + 8 significant bits), six MFMA products per MAC on
// v_mfma_f32_32x32x16_bf16, small products first (x1 w3, x3 w1, x2 w2, x1 w2, x2 w1, x1 w1; x2 w3, x3 w2, x3 w3 <= 2^-24 relative are dropped, as in the GEMM),
// float32 accumulation.  bf16 has float32's exponent: no weight pre-scaling, no activation range limit; NaN / Inf inputs give NaN.  Float32 NHWC in and out.
//
// The structure is k_conv3x3_x2's (vd3d_conv2.hip), on an LDS plan that fits three terms:
//   implicit GEMM per workgroup, M = 256 pixels = an 8 x 32 output tile (8 MFMA M tiles = the tile's rows), N = CK output channels, K = 9 taps x C_in in steps
//   of 16 channels.  512 threads = 8 waves as 4 (M: two tile rows each) x 2 (N), two accumulators per each of 2 x NWN tiles (CK = 64 NWN); for 32 output channels 8 (M) x 1 (N).
//   A (pixels): the input tile + 1 halo ring (10 x 34 = 340 pixels), ONE 16-channel chunk at a time, fetched ONCE by LDS-DMA into a float32 staging buffer (a
//     chunk ahead; pixels outside the image fetch the zero page), split once into LDS [term 3][k-half 2][pixel 340][8 bf16] (32 640 B, double-buffered); all
//     nine taps read their fragments from it: 32 consecutive pixels of a tile row shifted by the tap = consecutive 16-byte slots, conflict-free ds_read_b128.
//   B (weights): packed once per model into the dense K-step image [chunk][tap][term 3][k-half 2][oc C_out][8 bf16] (96 C_out bytes per step) and streamed
//     by LDS-DMA through a ring of NS stages, NS - 1 steps ahead, counted vmcnt + raw s_barrier.  A ring stage is [term][k-half][oc CK][8 bf16] in whole
//     8 KB DMA rounds; the lanes of a round's padding read the zero page (one cache line, no bandwidth).  A workgroup that computes CK of C_out channels
//     (C_out 256 as two 128-channel halves on blockIdx.z) gathers its six 16 CK-byte pieces of a step through the per-lane source address.
//   LDS: 2 x 32 640 + 24 576 (staging) + NS x stage = 122 624 (CK 32, 64: 4 x 8 192), 155 392 (CK 128: 4 x 16 384).
// Per K step and wave: 6 A + 3 NWN B ds_read_b128 feed 2 x NWN x 6 MFMAs.
#include <mutex>

#include "vd3d_dev.h"
#include "vd3d_kernels.h"

typedef short c3_s8 __attribute__((ext_vector_type(8)));
typedef __bf16 c3_b8 __attribute__((ext_vector_type(8)));
typedef float c3_f16 __attribute__((ext_vector_type(16)));
typedef uint32_t c3_u2 __attribute__((ext_vector_type(2)));

#define C3_TH 8
#define C3_TW 32
#define C3_PH (C3_TH + 2)
#define C3_PW (C3_TW + 2)
#define C3_NPIX (C3_PH * C3_PW)                       // 340
#define C3_NT 512
#define C3_PLANE (C3_NPIX * 16)                       // one (term, k-half) plane: 5 440 bytes
#define C3_A_BUF (3 * 2 * C3_PLANE)                   // one chunk image: 32 640 bytes
#define C3_A_ITEMS (C3_NPIX * 4)                      // (pixel, 4-channel quad) items of a chunk: 1 360
#define C3_A_ITERS ((C3_A_ITEMS + C3_NT - 1) / C3_NT) // 3 per thread
#define C3_A_STG (C3_A_ITERS * C3_NT * 16)            // float32 staging buffer of one chunk, item-linear (what a DMA instruction can write): 24 576 bytes
__host__ __device__ constexpr int c3_b_stage(int ck) { return (3 * 2 * ck * 16 + 8191) / 8192 * 8192; }   // 8 192 (32, 64), 16 384 (128)
#define C3_B_OFF (2 * C3_A_BUF + C3_A_STG)
__host__ __device__ constexpr int c3_lds(int ck, int ns) { return C3_B_OFF + ns * c3_b_stage(ck); }
#define C3_LDS_MAX 155392                             // the largest dynamic LDS request of any instantiation (CK 128, four stages); a workgroup can have 163 840
static_assert(c3_lds(128, 4) == C3_LDS_MAX && c3_lds(64, 4) <= C3_LDS_MAX && c3_lds(32, 4) <= C3_LDS_MAX && C3_LDS_MAX <= 163840, "LDS plan");

struct vd_c3_args {
  int B, H, W, Cin, Cout;   // Cout: all output channels (the row pitch of Y and of a weight plane)
  int ntx, nty;             // tiles per frame
  int nchunk;               // Cin / 16
};

typedef __attribute__((address_space(3))) void* c3_lds_vp;
typedef const __attribute__((address_space(1))) void* c3_glb_vp;

// gx_split of vd3d_gemm.hip: exact, a = t1 + t2 + t3 with the terms in the high halves of the words
__device__ __forceinline__ void c3_split(float a, uint32_t& t1, uint32_t& t2, uint32_t& t3) {
  t1 = __float_as_uint(a) & 0xffff0000u;
  const float r1 = a - __uint_as_float(t1);
  t2 = __float_as_uint(r1) & 0xffff0000u;
  const float r2 = r1 - __uint_as_float(t2);
  t3 = __float_as_uint(r2);   // <= 8 significant bits: its low half is zero
}
__device__ __forceinline__ uint32_t c3_pack(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

// WM waves along M (4: two tile rows each, two waves along N; 8: one row each, one along N), NWN N tiles per wave: CK = 32 (8 / WM) NWN channels per workgroup
// (blockIdx.z picks the CK-channel slice of C_out), NS ring stages.
template <int WM, int NWN, int NS>
__global__ __launch_bounds__(C3_NT) void k_conv3x3_x3(const float* __restrict__ X, const uint8_t* __restrict__ Wimg, const float* __restrict__ zero16,
                                                      float* __restrict__ Y, vd_c3_args a) {
  constexpr int WN = 8 / WM, MR = C3_TH / WM, CK = 32 * WN * NWN, BST = c3_b_stage(CK), NBP = BST / (C3_NT * 16), B_ITEMS = 6 * CK;
  constexpr int A_FLY = NS - 2;   // the taps of a chunk whose counted wait leaves the next chunk's pixel DMAs in flight
  extern __shared__ __attribute__((aligned(16))) uint8_t c3_smem[];   // the only LDS object: [A buffer 0][A buffer 1][float32 staging][B ring]
  const int tile = blockIdx.x, b = blockIdx.y, oc0 = blockIdx.z * CK;
  const int tyi = tile / a.ntx, txi = tile - tyi * a.ntx;
  const int y0 = tyi * C3_TH, x0 = txi * C3_TW;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - wm * WN, li = lane & 31, kh = lane >> 5;
  const int wave_base = (tid & ~63) * 16;

  // ---- A staging: item i = it * 512 + tid -> (pixel = i >> 2 of the 10 x 34 halo tile, quad = i & 3 = four of the chunk's 16 channels); the DMA of item i lands
  // in staging slot i.  A pixel outside the image (zero padding) or an item past the tile fetches the 64 zero bytes behind the weight image.
  const float* ap[C3_A_ITERS]; int adst[C3_A_ITERS]; bool azero[C3_A_ITERS];
#pragma unroll
  for (int it = 0; it < C3_A_ITERS; ++it) {
    const int i = it * C3_NT + tid, pix = i >> 2, q = i & 3;
    const int py = pix / C3_PW, px = pix - py * C3_PW;
    const int gy = y0 - 1 + py, gx = x0 - 1 + px;
    const bool in = i < C3_A_ITEMS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    azero[it] = !in;
    ap[it] = in ? X + (((size_t)b * a.H + gy) * a.W + gx) * a.Cin + q * 4 : zero16;
    adst[it] = i < C3_A_ITEMS ? ((q >> 1) * C3_NPIX + pix) * 16 + (q & 1) * 8 : -1;   // + term * 2 * C3_PLANE
  }
  auto load_a = [&](int chunk) {
#pragma unroll
    for (int it = 0; it < C3_A_ITERS; ++it)
      __builtin_amdgcn_global_load_lds((c3_glb_vp)(azero[it] ? ap[it] : ap[it] + chunk * 16),
                                       (c3_lds_vp)(c3_smem + 2 * C3_A_BUF + it * (C3_NT * 16) + wave_base), 16, 0, 0);
  };
  auto write_a = [&](int buf) {   // staging (float32) -> exact three-term split -> three 8-byte LDS stores per item
    uint8_t* dst = c3_smem + buf * C3_A_BUF;
    const uint8_t* stg = c3_smem + 2 * C3_A_BUF + tid * 16;
#pragma unroll
    for (int it = 0; it < C3_A_ITERS; ++it) {
      // read as a short vector and bit-cast: hipcc orders a float4 LDS read behind every LDS-DMA in flight (vmcnt(0)), not this type (vd3d_gemm.hip)
      const c3_s8 raw = *reinterpret_cast<const c3_s8*>(stg + it * (C3_NT * 16));
      const float4 f = __builtin_bit_cast(float4, raw);
      uint32_t t1[4], t2[4], t3[4];
      c3_split(f.x, t1[0], t2[0], t3[0]); c3_split(f.y, t1[1], t2[1], t3[1]); c3_split(f.z, t1[2], t2[2], t3[2]); c3_split(f.w, t1[3], t2[3], t3[3]);
      if (adst[it] >= 0) {
        *reinterpret_cast<c3_u2*>(dst + adst[it]) = c3_u2{c3_pack(t1[0], t1[1]), c3_pack(t1[2], t1[3])};
        *reinterpret_cast<c3_u2*>(dst + 2 * C3_PLANE + adst[it]) = c3_u2{c3_pack(t2[0], t2[1]), c3_pack(t2[2], t2[3])};
        *reinterpret_cast<c3_u2*>(dst + 4 * C3_PLANE + adst[it]) = c3_u2{c3_pack(t3[0], t3[1]), c3_pack(t3[2], t3[3])};
      }
    }
  };
  // ---- B staging: K step ks = chunk * 9 + tap of the packed image; item i = p * 512 + tid -> ((term, k-half) plane = i / CK, oc = i % CK) of this workgroup's
  // channel slice, NBP DMA instructions per thread; the items behind the stage's 6 CK read the zero page
  const uint8_t* bp[NBP]; bool bzero[NBP];
  const size_t bstep = (size_t)a.Cout * 96;
#pragma unroll
  for (int p = 0; p < NBP; ++p) {
    const int i = p * C3_NT + tid;
    bzero[p] = i >= B_ITEMS;
    bp[p] = bzero[p] ? reinterpret_cast<const uint8_t*>(zero16) : Wimg + ((size_t)(i / CK) * a.Cout + oc0 + (i % CK)) * 16;
  }
  auto stage_b = [&](int ks, int slot) {
#pragma unroll
    for (int p = 0; p < NBP; ++p)
      __builtin_amdgcn_global_load_lds((c3_glb_vp)(bzero[p] ? bp[p] : bp[p] + (size_t)ks * bstep),
                                       (c3_lds_vp)(c3_smem + C3_B_OFF + slot * BST + p * (C3_NT * 16) + wave_base), 16, 0, 0);
  };

  // Two accumulators per tile: x1 w1 in `acc`, the five correction products (<= 2^-7 of it) in `lo`, summed in the epilogue.  One float32 rounding at the
  // running sum's magnitude per K step instead of six: with a single accumulator the 1024-channel neck convolution (55 296 MFMA adds per output) measured a
  // relative RMS error 1.8 x that of a float32 CPU convolution, outside the bar of tests/test_hip_conv_x3.py.
  c3_f16 acc[MR][NWN], lo[MR][NWN];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NWN; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = lo[m][n][r] = 0.f;

  const int KS = a.nchunk * 9;
  load_a(0);
#pragma unroll
  for (int st = 0; st < NS - 1; ++st) stage_b(st < KS ? st : KS - 1, st);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prologue waits for everything; a thread converts only the staging slots its OWN DMA lanes filled
  write_a(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // fragment base offsets: A: k-half plane, tile row MR wm + m (+ 1 halo + dy), column li (+ 1 + dx); B: k-half plane, output channel (wn * NWN + n) * 32 + li
  const int fa_base = (kh * C3_NPIX + (MR * wm + 1) * C3_PW + li + 1) * 16;
  const int fb_base = C3_B_OFF + (kh * CK + wn * NWN * 32 + li) * 16;
  int ks = 0;
  for (int chunk = 0; chunk < a.nchunk; ++chunk) {
    const bool more_a = chunk + 1 < a.nchunk;   // uniform
    if (more_a) load_a(chunk + 1);
    const uint8_t* sa = c3_smem + (chunk & 1) * C3_A_BUF;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap, ++ks) {
      const int slot = ks % NS, dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
      stage_b(ks + NS - 1 < KS ? ks + NS - 1 : KS - 1, (ks + NS - 1) % NS);   // behind the last step: a harmless re-fetch (straight-line code, one counted wait)
      const uint8_t* sb = c3_smem + slot * BST;
      const uint8_t* sat = sa + fa_base + (dy * C3_PW + dx) * 16;
      c3_s8 af[MR][3];
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int t = 0; t < 3; ++t) af[m][t] = *reinterpret_cast<const c3_s8*>(sat + t * (2 * C3_PLANE) + m * (C3_PW * 16));
#pragma unroll
      for (int n = 0; n < NWN; ++n) {
        c3_s8 bf[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) bf[t] = *reinterpret_cast<const c3_s8*>(sb + fb_base + t * (2 * CK * 16) + n * 512);
        // small products first, into their own accumulator; the M tiles alternate so that dependent MFMAs are not back to back
#define C3_MM(ACC, ta, tb)                                                                                                                                \
  _Pragma("unroll") for (int m = 0; m < MR; ++m)                                                                                                          \
    ACC[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(c3_b8, af[m][ta]), __builtin_bit_cast(c3_b8, bf[tb]), ACC[m][n], 0, 0, 0);
        C3_MM(lo, 0, 2) C3_MM(lo, 2, 0) C3_MM(lo, 1, 1) C3_MM(lo, 0, 1) C3_MM(lo, 1, 0) C3_MM(acc, 0, 0)
#undef C3_MM
      }
      // Counted wait.  In flight, oldest first: [B (ks + 1)] .. [B (ks + NS - 2)] [B (ks + NS - 1)], with the next chunk's C3_A_ITERS pixel DMAs (issued in front of
      // tap 0's B round) between B (ks0 + NS - 2) and B (ks0 + NS - 1).  The next step needs B (ks + 1): through tap NS - 3 the pixel DMAs and the NS - 2 younger
      // B rounds stay in flight; from tap NS - 2 on the pixel DMAs are older than what must land, so they land too.
      if (more_a && tap < A_FLY) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * NBP + C3_A_ITERS) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * NBP) : "memory");
      if (more_a && tap == NS - 1) {   // the next chunk's pixels have landed (tap NS - 2's wait): split them into the other buffer -- last read in the previous chunk
        write_a((chunk + 1) & 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue: accumulator register r of (m, n) = pixel column (r & 3) + 8 (r >> 2) + 4 kh of tile row MR wm + m, output channel oc0 + (wn * NWN + n) * 32 + li
#pragma unroll
  for (int n = 0; n < NWN; ++n) {
    const int oc = oc0 + (wn * NWN + n) * 32 + li;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int y = y0 + MR * wm + m;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int x = x0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (y < a.H && x < a.W) Y[(((size_t)b * a.H + y) * a.W + x) * a.Cout + oc] = acc[m][n][r] + lo[m][n][r];
      }
    }
  }
}

// ---- weights: float32 [Cout][Cin][3][3] -> the dense K-step images [chunk][tap][term 3][k-half 2][oc][8 bf16]; one thread = (chunk, tap, k-half, oc): 8 channels
__global__ __launch_bounds__(256) void k_conv3x3_x3_pack(const float* __restrict__ W, int Cout, int Cin, uint8_t* __restrict__ img) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int nchunk = Cin / 16, total = nchunk * 9 * 2 * Cout;
  if (t >= total) return;
  const int oc = t % Cout, khf = (t / Cout) & 1, tap = (t / (2 * Cout)) % 9, chunk = t / (18 * Cout);
  uint32_t t1[8], t2[8], t3[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) c3_split(W[((size_t)oc * Cin + chunk * 16 + khf * 8 + e) * 9 + tap], t1[e], t2[e], t3[e]);
  uint8_t* base = img + (size_t)(chunk * 9 + tap) * Cout * 96 + (khf * Cout + oc) * 16;
  *reinterpret_cast<uint4*>(base) = make_uint4(c3_pack(t1[0], t1[1]), c3_pack(t1[2], t1[3]), c3_pack(t1[4], t1[5]), c3_pack(t1[6], t1[7]));
  *reinterpret_cast<uint4*>(base + 2 * Cout * 16) = make_uint4(c3_pack(t2[0], t2[1]), c3_pack(t2[2], t2[3]), c3_pack(t2[4], t2[5]), c3_pack(t2[6], t2[7]));
  *reinterpret_cast<uint4*>(base + 4 * Cout * 16) = make_uint4(c3_pack(t3[0], t3[1]), c3_pack(t3[2], t3[3]), c3_pack(t3[4], t3[5]), c3_pack(t3[6], t3[7]));
}

static bool c3_shape_ok(int Cin, int Cout) { return Cin >= 16 && (Cin & 15) == 0 && (Cout == 32 || Cout == 64 || Cout == 128 || Cout == 256); }
long long vd_conv3x3_x3_weight_bytes(int Cin, int Cout) {
  if (!c3_shape_ok(Cin, Cout)) return -1;
  return (long long)(Cin / 16) * 9 * Cout * 96 + 64;   // step images, 64 zero bytes (the zero page of the padding)
}
bool vd_launch_conv3x3_x3_pack(hipStream_t s, const float* W, int Cin, int Cout, void* img) {
  const long long nb = vd_conv3x3_x3_weight_bytes(Cin, Cout);
  if (nb < 0 || (reinterpret_cast<uintptr_t>(img) & 15)) return false;
  if (hipMemsetAsync(reinterpret_cast<uint8_t*>(img) + nb - 64, 0, 64, s) != hipSuccess) return false;
  const int total = (Cin / 16) * 9 * 2 * Cout;
  hipLaunchKernelGGL(k_conv3x3_x3_pack, dim3((total + 255) / 256), dim3(256), 0, s, W, Cout, Cin, reinterpret_cast<uint8_t*>(img));
  return true;
}

// 256 output channels run as two 128-channel halves on blockIdx.z (each fetches and splits the input tile): one workgroup with all 256 channels would need
// 2 x 128 accumulator registers for the two-accumulator sum above, which two waves per SIMD do not have.
bool vd_launch_conv3x3_x3(hipStream_t s, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, float* Y) {
  const long long nb = vd_conv3x3_x3_weight_bytes(Cin, Cout);
  if (nb < 0 || B < 1 || H < 1 || W < 1 || B > 65535) return false;
  if ((reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(wimg) & 15) || (reinterpret_cast<uintptr_t>(Y) & 3)) return false;
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_conv3x3_x3<8, 1, 4>), c3_lds(32, 4)}, {reinterpret_cast<const void*>(k_conv3x3_x3<4, 1, 4>), c3_lds(64, 4)},
                     {reinterpret_cast<const void*>(k_conv3x3_x3<4, 2, 4>), c3_lds(128, 4)}}, attr_set)) return false;
  vd_c3_args a;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.ntx = (W + C3_TW - 1) / C3_TW; a.nty = (H + C3_TH - 1) / C3_TH; a.nchunk = Cin / 16;
  const uint8_t* wi = reinterpret_cast<const uint8_t*>(wimg);
  const float* z16 = reinterpret_cast<const float*>(wi + nb - 64);
  const dim3 grid((unsigned)(a.ntx * a.nty), (unsigned)B, 1);
  if (Cout == 32) hipLaunchKernelGGL((k_conv3x3_x3<8, 1, 4>), grid, dim3(C3_NT), c3_lds(32, 4), s, X, wi, z16, Y, a);   // the head's 64 -> 32
  else if (Cout == 64) hipLaunchKernelGGL((k_conv3x3_x3<4, 1, 4>), grid, dim3(C3_NT), c3_lds(64, 4), s, X, wi, z16, Y, a);
  else if (Cout == 128) hipLaunchKernelGGL((k_conv3x3_x3<4, 2, 4>), grid, dim3(C3_NT), c3_lds(128, 4), s, X, wi, z16, Y, a);
  else hipLaunchKernelGGL((k_conv3x3_x3<4, 2, 4>), dim3(grid.x, grid.y, 2), dim3(C3_NT), c3_lds(128, 4), s, X, wi, z16, Y, a);
  return true;
}
