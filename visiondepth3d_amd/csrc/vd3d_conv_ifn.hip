// vd3d_conv_ifn.hip -- the convolutions of the RIFE interpolation network (IFNet HDv3: three IFBlocks of 14 convolutions) in the bf16x3 arithmetic of
// vd3d_conv3.hip, and the float32 glue between its blocks (warp + down-scale + concatenate, flow / mask update, final blend).
//
// Arithmetic: k_conv3x3_x3's.  Every float32 operand is split EXACTLY into three bf16 terms by truncation (cf_split), the products x1 w3, x3 w1, x2 w2, x1 w2,
// x2 w1 go into a `lo` accumulator and x1 w1 into `acc` (v_mfma_f32_32x32x16_bf16, float32 accumulation), summed in the epilogue.  Float32 NHWC in and out,
// NaN / Inf in gives NaN out, no range limit.
//
// One kernel, three geometries (template parameter KIND), all on k_conv3x3_x3's LDS plan: an 8 x 32 tile of the "tile grid" per 512-thread workgroup, its
// 10 x 34 halo tile staged one 16-channel chunk at a time by LDS-DMA (float32 staging buffer, a chunk ahead, the zero page for pixels outside the image), split
// once into [term 3][k-half 2][pixel 340][8 bf16] (double-buffered), weights streamed through a four-stage LDS ring, counted vmcnt + raw s_barrier.
//   K3S1  3 x 3, stride 1, padding 1.  Tile grid = output = input.  9 K steps per chunk (tap (dy, dx) = a shift of the fragment address).
//   K3S2  3 x 3, stride 2, padding 1, output (H+1)/2 x (W+1)/2.  The space-to-depth view WITHOUT zero-filled taps: tile grid = output; a staged "chunk" is
//         (16 channels, sub-pixel (sy, sx)) and holds input pixel (2 ty + sy, 2 tx + sx) at tile position (ty, tx).  Output (q, r) reads input rows 2q-1, 2q,
//         2q+1: sub-row 0 serves k_y = 1 at dy = 0, sub-row 1 serves k_y = 0 at dy = -1 and k_y = 2 at dy = 0; the same in x.  So the four sub-pixels run
//         1, 2, 2 and 4 K steps: 9 per 16 channels, no MFMA on zero weights (a zero-weight tap would also carry a NaN to outputs whose window does not hold it).
//         The price is four stagings per 16 channels; this geometry is about 6 % of the network's MACs.
//   T4S2  ConvTranspose2d(4, stride 2, padding 1), output 2H x 2W, as four output phases, each a 2 x 2 stride-1 convolution of the input: phase p = 0 takes
//         k = 3 at i = q - 1 and k = 1 at i = q, phase p = 1 takes k = 2 at i = q and k = 0 at i = q + 1 (the same in x); output pixel (2q + p_y, 2r + p_x).
//         Tile grid = input.  The phase is blockIdx.z: each workgroup stages the tile and runs 4 K steps per chunk.  (All four phases from one staged tile
//         would need 4 x the accumulators: 384 registers at 96 output channels.)
// Channels: C_in a multiple of 16 read from pixels of pitch x_stride; C_out = CK in {32, 64, 96} written at [y_offset, y_offset + C_out) of pixels of pitch
// y_stride.  Waves: 8 (M) x 1 (N) with 1 (C_out 32) or 3 (C_out 96) N tiles per wave, 4 (M) x 2 (N) for C_out 64: 32 / 64 / 96 accumulator registers x 2.
// Epilogue (float32): y = acc + lo + bias[oc]; y = y >= 0 ? y : slope[oc] * y (slope == nullptr: none); y += R[pixel][oc] (R == nullptr: none).
// LDS: 2 x 32 640 + 24 576 + 4 x stage (8 192 for C_out 32 / 64, 16 384 for 96) = 122 624 / 155 392 bytes.
#include "vd3d_dev.h"
#include "vd3d_kernels.h"

typedef short cf_s8 __attribute__((ext_vector_type(8)));
typedef __bf16 cf_b8 __attribute__((ext_vector_type(8)));
typedef float cf_f16 __attribute__((ext_vector_type(16)));
typedef uint32_t cf_u2 __attribute__((ext_vector_type(2)));

#define CF_TH 8
#define CF_TW 32
#define CF_PH (CF_TH + 2)
#define CF_PW (CF_TW + 2)
#define CF_NPIX (CF_PH * CF_PW)                       // 340
#define CF_NT 512
#define CF_NS 4                                       // weight ring stages
#define CF_PLANE (CF_NPIX * 16)                       // one (term, k-half) plane: 5 440 bytes
#define CF_A_BUF (3 * 2 * CF_PLANE)                   // one chunk image: 32 640 bytes
#define CF_A_ITEMS (CF_NPIX * 4)                      // (pixel, 4-channel quad) items of a chunk: 1 360
#define CF_A_ITERS ((CF_A_ITEMS + CF_NT - 1) / CF_NT) // 3 per thread
#define CF_A_STG (CF_A_ITERS * CF_NT * 16)            // float32 staging buffer of one chunk: 24 576 bytes
__host__ __device__ constexpr int cf_b_stage(int ck) { return (3 * 2 * ck * 16 + 8191) / 8192 * 8192; }   // 8 192 (32, 64), 16 384 (96)
#define CF_B_OFF (2 * CF_A_BUF + CF_A_STG)
__host__ __device__ constexpr int cf_lds(int ck) { return CF_B_OFF + CF_NS * cf_b_stage(ck); }
#define CF_LDS_MAX 155392                             // the largest dynamic LDS request of any instantiation (C_out 96); a workgroup can have 163 840
static_assert(cf_lds(96) == CF_LDS_MAX && cf_lds(64) <= CF_LDS_MAX && cf_lds(32) <= CF_LDS_MAX && CF_LDS_MAX <= 163840, "LDS plan");

enum { CF_K3S1 = 0, CF_K3S2 = 1, CF_T4S2 = 2 };

struct vd_cf_args {
  const float* X; const uint8_t* Wimg; const float* zero16; const float* bias; const float* slope; const float* R; float* Y;
  int B, H, W;              // the input map
  int Ho, Wo;               // the output map
  int x_stride, y_stride, y_offset, r_stride;
  int ntx;                  // tiles per row of the tile grid
  int nchunk;               // C_in / 16
};

typedef __attribute__((address_space(3))) void* cf_lds_vp;
typedef const __attribute__((address_space(1))) void* cf_glb_vp;

// c3_split of vd3d_conv3.hip: exact, a = t1 + t2 + t3 with the terms in the high halves of the words
__device__ __forceinline__ void cf_split(float a, uint32_t& t1, uint32_t& t2, uint32_t& t3) {
  t1 = __float_as_uint(a) & 0xffff0000u;
  const float r1 = a - __uint_as_float(t1);
  t2 = __float_as_uint(r1) & 0xffff0000u;
  const float r2 = r1 - __uint_as_float(t2);
  t3 = __float_as_uint(r2);   // <= 8 significant bits: its low half is zero
}
__device__ __forceinline__ uint32_t cf_pack(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

template <int KIND, int WM, int NWN>
__global__ __launch_bounds__(CF_NT) void k_conv_ifn_x3(const vd_cf_args a) {
  constexpr int NS = CF_NS, WN = 8 / WM, MR = CF_TH / WM, CK = 32 * WN * NWN, BST = cf_b_stage(CK), NBP = BST / (CF_NT * 16), B_ITEMS = 6 * CK;
  constexpr int A_FLY = NS - 2;   // the taps of a chunk whose counted wait leaves the next chunk's pixel DMAs in flight
  constexpr int SUBS = KIND == CF_K3S2 ? 4 : 1, ST = KIND == CF_K3S2 ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) uint8_t cf_smem[];   // the only LDS object: [A buffer 0][A buffer 1][float32 staging][B ring]
  const int tile = blockIdx.x, b = blockIdx.y;
  const int ph_y = KIND == CF_T4S2 ? (int)(blockIdx.z >> 1) : 0, ph_x = KIND == CF_T4S2 ? (int)(blockIdx.z & 1) : 0;
  const int tyi = tile / a.ntx, txi = tile - tyi * a.ntx;
  const int y0 = tyi * CF_TH, x0 = txi * CF_TW;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - wm * WN, li = lane & 31, kh = lane >> 5;
  const int wave_base = (tid & ~63) * 16;

  // ---- A staging: item i = it * 512 + tid -> (pixel = i >> 2 of the 10 x 34 halo tile, quad = i & 3 = four of the chunk's 16 channels); the DMA of item i lands
  // in staging slot i.  A pixel outside the image (zero padding) or an item past the tile fetches the 64 zero bytes behind the weight image.
  int aty[CF_A_ITERS], atx[CF_A_ITERS], adst[CF_A_ITERS];
  const int q4 = tid & 3;
#pragma unroll
  for (int it = 0; it < CF_A_ITERS; ++it) {
    const int i = it * CF_NT + tid, pix = i >> 2;
    const int py = pix / CF_PW, px = pix - py * CF_PW;
    aty[it] = i < CF_A_ITEMS ? y0 - 1 + py : -(1 << 28);   // an item past the tile is "above the image"
    atx[it] = x0 - 1 + px;
    adst[it] = i < CF_A_ITEMS ? ((q4 >> 1) * CF_NPIX + pix) * 16 + (q4 & 1) * 8 : -1;   // + term * 2 * CF_PLANE
  }
  const float* xb = a.X + (size_t)b * a.H * a.W * a.x_stride + q4 * 4;
  auto load_a = [&](int chunk) {   // chunk = c16 * SUBS + (sy * 2 + sx)
    const int c16 = chunk / SUBS, sy = KIND == CF_K3S2 ? (chunk >> 1) & 1 : 0, sx = KIND == CF_K3S2 ? chunk & 1 : 0;
#pragma unroll
    for (int it = 0; it < CF_A_ITERS; ++it) {
      const int gy = ST * aty[it] + sy, gx = ST * atx[it] + sx;
      const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      const float* p = in ? xb + ((size_t)gy * a.W + gx) * a.x_stride + c16 * 16 : a.zero16;
      __builtin_amdgcn_global_load_lds((cf_glb_vp)p, (cf_lds_vp)(cf_smem + 2 * CF_A_BUF + it * (CF_NT * 16) + wave_base), 16, 0, 0);
    }
  };
  auto write_a = [&](int buf) {   // staging (float32) -> exact three-term split -> three 8-byte LDS stores per item
    uint8_t* dst = cf_smem + buf * CF_A_BUF;
    const uint8_t* stg = cf_smem + 2 * CF_A_BUF + tid * 16;
#pragma unroll
    for (int it = 0; it < CF_A_ITERS; ++it) {
      // read as a short vector and bit-cast: hipcc orders a float4 LDS read behind every LDS-DMA in flight (vmcnt(0)), not this type (vd3d_gemm.hip)
      const cf_s8 raw = *reinterpret_cast<const cf_s8*>(stg + it * (CF_NT * 16));
      const float4 f = __builtin_bit_cast(float4, raw);
      uint32_t t1[4], t2[4], t3[4];
      cf_split(f.x, t1[0], t2[0], t3[0]); cf_split(f.y, t1[1], t2[1], t3[1]); cf_split(f.z, t1[2], t2[2], t3[2]); cf_split(f.w, t1[3], t2[3], t3[3]);
      if (adst[it] >= 0) {
        *reinterpret_cast<cf_u2*>(dst + adst[it]) = cf_u2{cf_pack(t1[0], t1[1]), cf_pack(t1[2], t1[3])};
        *reinterpret_cast<cf_u2*>(dst + 2 * CF_PLANE + adst[it]) = cf_u2{cf_pack(t2[0], t2[1]), cf_pack(t2[2], t2[3])};
        *reinterpret_cast<cf_u2*>(dst + 4 * CF_PLANE + adst[it]) = cf_u2{cf_pack(t3[0], t3[1]), cf_pack(t3[2], t3[3])};
      }
    }
  };
  // ---- B staging: the packed image holds the K steps in the order this kernel runs them, [step][term 3][k-half 2][oc CK][8 bf16]; item i = p * 512 + tid is
  // 16 bytes of a step; the items behind the step's 96 CK bytes read the zero page
  const int NCH = a.nchunk * SUBS;
  const int KS = KIND == CF_T4S2 ? a.nchunk * 4 : a.nchunk * 9;
  const size_t bstep = (size_t)CK * 96;
  const uint8_t* wbase = a.Wimg + (KIND == CF_T4S2 ? (size_t)(ph_y * 2 + ph_x) * KS * bstep : (size_t)0);
  auto stage_b = [&](int ks, int slot) {
#pragma unroll
    for (int p = 0; p < NBP; ++p) {
      const int i = p * CF_NT + tid;
      const uint8_t* src = i < B_ITEMS ? wbase + (size_t)ks * bstep + i * 16 : reinterpret_cast<const uint8_t*>(a.zero16);
      __builtin_amdgcn_global_load_lds((cf_glb_vp)src, (cf_lds_vp)(cf_smem + CF_B_OFF + slot * BST + p * (CF_NT * 16) + wave_base), 16, 0, 0);
    }
  };

  cf_f16 acc[MR][NWN], lo[MR][NWN];   // x1 w1 in `acc`, the five correction products in `lo` (vd3d_conv3.hip)
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
  const int fa_base = (kh * CF_NPIX + (MR * wm + 1) * CF_PW + li + 1) * 16;
  const int fb_base = CF_B_OFF + (kh * CK + wn * NWN * 32 + li) * 16;
  int ks = 0;
  for (int chunk = 0; chunk < NCH; ++chunk) {
    const bool more_a = chunk + 1 < NCH;   // uniform
    if (more_a) load_a(chunk + 1);
    const uint8_t* sa = cf_smem + (chunk & 1) * CF_A_BUF;
    const int sy = KIND == CF_K3S2 ? (chunk >> 1) & 1 : 0, sx = KIND == CF_K3S2 ? chunk & 1 : 0;
    const int T = KIND == CF_K3S1 ? 9 : KIND == CF_T4S2 ? 4 : (1 + sy) * (1 + sx);
#pragma unroll 1
    for (int tap = 0; tap < T; ++tap, ++ks) {
      int dy, dx;
      if (KIND == CF_K3S1) { dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
      else if (KIND == CF_T4S2) { dy = ph_y + (tap >> 1) - 1; dx = ph_x + (tap & 1) - 1; }
      else { const int ty = sx ? tap >> 1 : tap, tx = sx ? tap & 1 : 0; dy = ty - sy; dx = tx - sx; }
      const int slot = ks % NS;
      stage_b(ks + NS - 1 < KS ? ks + NS - 1 : KS - 1, (ks + NS - 1) % NS);   // behind the last step: a harmless re-fetch (straight-line code, one counted wait)
      const uint8_t* sb = cf_smem + slot * BST;
      const uint8_t* sat = sa + fa_base + (dy * CF_PW + dx) * 16;
      cf_s8 af[MR][3];
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int t = 0; t < 3; ++t) af[m][t] = *reinterpret_cast<const cf_s8*>(sat + t * (2 * CF_PLANE) + m * (CF_PW * 16));
#pragma unroll
      for (int n = 0; n < NWN; ++n) {
        cf_s8 bf[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) bf[t] = *reinterpret_cast<const cf_s8*>(sb + fb_base + t * (2 * CK * 16) + n * 512);
#define CF_MM(ACC, ta, tb)                                                                                                                                \
  _Pragma("unroll") for (int m = 0; m < MR; ++m)                                                                                                          \
    ACC[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cf_b8, af[m][ta]), __builtin_bit_cast(cf_b8, bf[tb]), ACC[m][n], 0, 0, 0);
        CF_MM(lo, 0, 2) CF_MM(lo, 2, 0) CF_MM(lo, 1, 1) CF_MM(lo, 0, 1) CF_MM(lo, 1, 0) CF_MM(acc, 0, 0)
#undef CF_MM
      }
      // Counted wait.  In flight, oldest first: B (ks + 1) .. B (ks + NS - 1), with the next chunk's CF_A_ITERS pixel DMAs issued in front of this chunk's tap 0
      // B round.  The next step needs B (ks + 1): while fewer than NS - 1 B rounds have followed the pixel DMAs (tap < NS - 2) they are younger than B (ks + 1)
      // and stay in flight with the NS - 2 younger B rounds; from tap NS - 2 on they are older than what must land, so they land too.
      if (more_a && tap < A_FLY) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * NBP + CF_A_ITERS) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NS - 2) * NBP) : "memory");
      if (more_a && tap == T - 1) {   // the chunk's last step: split the next chunk's pixels into the other buffer (last read in the previous chunk)
        if (KIND == CF_K3S2 && T < NS - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a 1- or 2-step chunk: the pixel DMAs have not been waited for yet
        write_a((chunk + 1) & 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue: accumulator register r of (m, n) = tile column (r & 3) + 8 (r >> 2) + 4 kh of tile row MR wm + m, output channel (wn * NWN + n) * 32 + li
#pragma unroll
  for (int n = 0; n < NWN; ++n) {
    const int oc = (wn * NWN + n) * 32 + li;
    const float bv = a.bias[oc], sv = a.slope ? a.slope[oc] : 1.f;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int ty = y0 + MR * wm + m;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tx = x0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int oy = KIND == CF_T4S2 ? 2 * ty + ph_y : ty, ox = KIND == CF_T4S2 ? 2 * tx + ph_x : tx;
        if (oy < a.Ho && ox < a.Wo) {
          const size_t pix = ((size_t)b * a.Ho + oy) * a.Wo + ox;
          float v = acc[m][n][r] + lo[m][n][r] + bv;
          if (a.slope) v = v >= 0.f ? v : sv * v;
          if (a.R) v += a.R[pix * a.r_stride + oc];
          a.Y[pix * a.y_stride + a.y_offset + oc] = v;
        }
      }
    }
  }
}

// ---- weights -> the K-step images [step][term 3][k-half 2][oc][8 bf16] in the order the kernel runs the steps; one thread = (step, k-half, oc): 8 channels.
// K3S1 / K3S2: W[Cout][Cin][3][3]; T4S2: W[Cin][Cout][4][4] (PyTorch's layouts).
__global__ __launch_bounds__(256) void k_conv_ifn_pack(int kind, const float* __restrict__ W, int Cout, int Cin, uint8_t* __restrict__ img) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int nchunk = Cin / 16, spc = kind == CF_T4S2 ? 16 : 9, total = nchunk * spc * 2 * Cout;
  if (t >= total) return;
  const int oc = t % Cout, khf = (t / Cout) & 1, step = t / (2 * Cout);
  int c16, ky, kx;
  if (kind == CF_K3S1) { c16 = step / 9; const int tap = step - c16 * 9; ky = tap / 3; kx = tap - ky * 3; }
  else if (kind == CF_K3S2) {   // per 16 channels: sub-pixel (0,0) 1 step, (0,1) 2, (1,0) 2, (1,1) 4
    c16 = step / 9;
    const int j = step - c16 * 9;
    const int sub = j == 0 ? 0 : j < 3 ? 1 : j < 5 ? 2 : 3, tap = j == 0 ? 0 : j < 3 ? j - 1 : j < 5 ? j - 3 : j - 5;
    const int sy = sub >> 1, sx = sub & 1, ty = sx ? tap >> 1 : tap, tx = sx ? tap & 1 : 0;
    ky = sy ? 2 * ty : 1; kx = sx ? 2 * tx : 1;
  } else {                      // [phase 4][chunk][tap 4]
    const int phase = step / (nchunk * 4), rem = step - phase * (nchunk * 4);
    c16 = rem >> 2;
    const int tap = rem & 3;
    ky = 3 - (phase >> 1) - 2 * (tap >> 1); kx = 3 - (phase & 1) - 2 * (tap & 1);
  }
  uint32_t t1[8], t2[8], t3[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ci = c16 * 16 + khf * 8 + e;
    const float w = kind == CF_T4S2 ? W[(((size_t)ci * Cout + oc) * 4 + ky) * 4 + kx] : W[(((size_t)oc * Cin + ci) * 3 + ky) * 3 + kx];
    cf_split(w, t1[e], t2[e], t3[e]);
  }
  uint8_t* base = img + (size_t)step * Cout * 96 + (khf * Cout + oc) * 16;
  *reinterpret_cast<uint4*>(base) = make_uint4(cf_pack(t1[0], t1[1]), cf_pack(t1[2], t1[3]), cf_pack(t1[4], t1[5]), cf_pack(t1[6], t1[7]));
  *reinterpret_cast<uint4*>(base + 2 * Cout * 16) = make_uint4(cf_pack(t2[0], t2[1]), cf_pack(t2[2], t2[3]), cf_pack(t2[4], t2[5]), cf_pack(t2[6], t2[7]));
  *reinterpret_cast<uint4*>(base + 4 * Cout * 16) = make_uint4(cf_pack(t3[0], t3[1]), cf_pack(t3[2], t3[3]), cf_pack(t3[4], t3[5]), cf_pack(t3[6], t3[7]));
}

long long vd_conv_ifn_weight_bytes(int kind, int Cin, int Cout) {
  if (kind < CF_K3S1 || kind > CF_T4S2 || Cin < 16 || (Cin & 15) || Cin > 65536 || (Cout != 32 && Cout != 64 && Cout != 96)) return -1;
  return (long long)(Cin / 16) * (kind == CF_T4S2 ? 16 : 9) * Cout * 96 + 64;   // step images, 64 zero bytes (the zero page of the padding)
}
bool vd_launch_conv_ifn_pack(hipStream_t s, int kind, const float* W, int Cin, int Cout, void* img) {
  const long long nb = vd_conv_ifn_weight_bytes(kind, Cin, Cout);
  if (nb < 0 || (reinterpret_cast<uintptr_t>(img) & 15)) return false;
  if (hipMemsetAsync(reinterpret_cast<uint8_t*>(img) + nb - 64, 0, 64, s) != hipSuccess) return false;
  const int total = (Cin / 16) * (kind == CF_T4S2 ? 16 : 9) * 2 * Cout;
  hipLaunchKernelGGL(k_conv_ifn_pack, dim3((total + 255) / 256), dim3(256), 0, s, kind, W, Cout, Cin, reinterpret_cast<uint8_t*>(img));
  return true;
}

template <int KIND>
static void cf_launch_kind(hipStream_t s, dim3 grid, int Cout, const vd_cf_args& a) {
  if (Cout == 32) hipLaunchKernelGGL((k_conv_ifn_x3<KIND, 8, 1>), grid, dim3(CF_NT), cf_lds(32), s, a);
  else if (Cout == 64) hipLaunchKernelGGL((k_conv_ifn_x3<KIND, 4, 1>), grid, dim3(CF_NT), cf_lds(64), s, a);
  else hipLaunchKernelGGL((k_conv_ifn_x3<KIND, 8, 3>), grid, dim3(CF_NT), cf_lds(96), s, a);
}

// The entry point (vd3d_conv_ifn) has checked every argument; false: the dynamic-LDS attribute could not be set.
bool vd_launch_conv_ifn(hipStream_t s, int kind, const float* X, int B, int H, int W, int x_stride, int Cin, const void* wimg, const float* bias,
                        const float* slope, int Cout, const float* R, int r_stride, float* Y, int y_stride, int y_offset) {
  const long long nb = vd_conv_ifn_weight_bytes(kind, Cin, Cout);
  if (nb < 0 || B < 1 || B > 65535 || H < 1 || W < 1) return false;
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
#define CF_FN(K) {reinterpret_cast<const void*>(k_conv_ifn_x3<K, 8, 1>), cf_lds(32)}, {reinterpret_cast<const void*>(k_conv_ifn_x3<K, 4, 1>), cf_lds(64)}, \
                 {reinterpret_cast<const void*>(k_conv_ifn_x3<K, 8, 3>), cf_lds(96)}
  if (!vd_lds_optin({CF_FN(CF_K3S1), CF_FN(CF_K3S2), CF_FN(CF_T4S2)}, attr_set)) return false;
#undef CF_FN
  vd_cf_args a;
  const uint8_t* wi = reinterpret_cast<const uint8_t*>(wimg);
  a.X = X; a.Wimg = wi; a.zero16 = reinterpret_cast<const float*>(wi + nb - 64); a.bias = bias; a.slope = slope; a.R = R; a.Y = Y;
  a.B = B; a.H = H; a.W = W;
  a.Ho = kind == CF_K3S2 ? (H + 1) / 2 : kind == CF_T4S2 ? 2 * H : H;
  a.Wo = kind == CF_K3S2 ? (W + 1) / 2 : kind == CF_T4S2 ? 2 * W : W;
  a.x_stride = x_stride; a.y_stride = y_stride; a.y_offset = y_offset; a.r_stride = r_stride; a.nchunk = Cin / 16;
  const int gh = kind == CF_K3S2 ? a.Ho : H, gw = kind == CF_K3S2 ? a.Wo : W;   // the tile grid
  a.ntx = (gw + CF_TW - 1) / CF_TW;
  const dim3 grid((unsigned)(a.ntx * ((gh + CF_TH - 1) / CF_TH)), (unsigned)B, kind == CF_T4S2 ? 4u : 1u);
  if (kind == CF_K3S1) cf_launch_kind<CF_K3S1>(s, grid, Cout, a);
  else if (kind == CF_K3S2) cf_launch_kind<CF_K3S2>(s, grid, Cout, a);
  else cf_launch_kind<CF_T4S2>(s, grid, Cout, a);
  return true;
}

// =====================================================================================================================================================
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
