// vd3d_conv_poly.hip -- the neck's transposed convolution (kernel == stride == F, with bias) and the 3 x 3 convolution behind it (padding 1, no bias) as ONE
// exact-float32 kernel on the COARSE map, in polyphase form:
//
//     out[b][F i + pa][F j + pb][:] = sum over the offsets (di, dj) phase (pa, pb) reaches, in block order, of  Wc[k] x[b][i + di][j + dj][:]  (+ bc[k])
//
// The transposed convolution writes F x F fine pixels per coarse pixel, each from that one pixel, and nothing non-linear sits between the two layers: a 3 x 3
// window of the fine map sees 2 x 2 coarse pixels at most.  The composed matrices Wc[k] [C_OUT][C_IN] and bias vectors bc[k] [C_OUT] come from the host (float64,
// rounded once: depth.py neck_poly_compose).  Block order k (the order of every sum): phase row pa, phase column pb, then di ascending, dj ascending, where phase
// coordinate 0 reaches {-1, 0}, F - 1 reaches {0, 1} and every other one {0}: (F + 2)^2 blocks, 36 for F = 4 and 16 for F = 2.  A coarse pixel outside the map
// contributes nothing, neither its product nor its bias: the 3 x 3 convolution pads the FINE map with zeros.  The fine map [F h][F w][C] is never written.
//
// Arithmetic: float32 operands on v_mfma_f32_32x32x2_f32, float32 accumulation (k_conv3x3_up_f32's class).  No split-K, no atomics; every output element is summed
// by one lane in one fixed order, so a frame's bits depend neither on the batch nor on the call:
//     per block a fresh accumulator: slots s of KS channels ascending, step st = 0 .. KS / 8 - 1, component c = 0 .. 3; one MFMA sums channel
//         s KS + 4 st + c (k = 0) and s KS + KS / 2 + 4 st + c (k = 1);
//     total = total + block, blocks ascending (blocked summation: chains of C_IN / 2 steps whose sums meet in at most four additions);
//     then total = total + bc[k] for the blocks of the phase whose coarse pixel lies inside the map, ascending.
//
// Work: a wave = 32 consecutive pixels of the flat coarse pixel list [B h w] (the MFMA's N side; no tile geometry, so no padding lanes but the list's tail), all C_OUT
// channels (M side, C_OUT / 32 accumulator tiles).  A lane reads its B operand -- KS / 2 consecutive channels of ITS neighbour pixel, 16-byte loads, a slot ahead --
// straight from global memory (the coarse map is small and L2-resident; a lane outside the map keeps an in-bounds address and selects 0).  A workgroup = 4 waves = 128
// pixels x one phase (blockIdx.y, phases in descending cost); its blocks' weights stream through a double-buffered LDS slot (registers -> LDS a slot ahead, one
// barrier per slot), A fragments by ds_read_b128.  Weight image: [block][slot][st][k-half 2][oc C_OUT][4 floats].
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include "vd3d_x3.h"

typedef float cp_f4 __attribute__((ext_vector_type(4)));

#define CP_NT 256
#define CP_PIX 128       // pixels of a workgroup
#define CP_MAXBLK 36
#define CP_MAXPH 16

__host__ __device__ constexpr int cp_ks(int cin) { return cin % 32 == 0 ? 32 : 16; }                            // channels of a weight slot
__host__ __device__ constexpr int cp_slot_floats(int cin, int cout) { return cp_ks(cin) / 8 * 2 * cout * 4; }   // 16 384 bytes for 32 channels x 128
__host__ __device__ constexpr int cp_nblk(int f) { return (f + 2) * (f + 2); }

struct vd_cp_args {
  int h, w, npix;                    // the coarse map; B h w
  int kbeg[CP_MAXPH], kend[CP_MAXPH];   // per blockIdx.y: the blocks of one phase
  int pa[CP_MAXPH], pb[CP_MAXPH];   // (ints: a uniform index reads them with scalar loads)
  int di[CP_MAXBLK], dj[CP_MAXBLK];
};

template <int C_IN, int C_OUT, int F>
__global__ __launch_bounds__(CP_NT) void k_conv_poly_f32(const float* __restrict__ X, const float* __restrict__ Wimg, const float* __restrict__ bc,
                                                         float* __restrict__ out, vd_cp_args a) {
  constexpr int KS = cp_ks(C_IN), NSLOT = C_IN / KS, ST = KS / 8, NM = C_OUT / 32, SLOT_F = cp_slot_floats(C_IN, C_OUT), W_ITERS = SLOT_F / 4 / CP_NT;
  static_assert(C_IN % KS == 0 && C_OUT % 32 == 0 && W_ITERS * CP_NT * 4 == SLOT_F && 2 * SLOT_F * 4 <= 65536, "slot plan");
  __shared__ __attribute__((aligned(16))) float cp_w[2][SLOT_F];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kh = lane >> 5;
  const int P = blockIdx.x * CP_PIX + wave * 32 + li;
  const bool live = P < a.npix;
  const int Pc = live ? P : 0;            // every address below is formed from an in-map pixel
  const int hw = a.h * a.w, bi = Pc / hw, rem = Pc - bi * hw, i = rem / a.w, j = rem - i * a.w;
  const int ph = blockIdx.y, kbeg = a.kbeg[ph], kend = a.kend[ph];
  const int T = (kend - kbeg) * NSLOT;

  cp_f4 xn[ST], xc[ST], wn[W_ITERS];
  bool vn;
  auto inside = [&](int k) { return live && (unsigned)(i + a.di[k]) < (unsigned)a.h && (unsigned)(j + a.dj[k]) < (unsigned)a.w; };
  auto load = [&](int t) {   // slot t of this workgroup: the lane's B operand and the thread's share of the weights
    const int k = kbeg + t / NSLOT, s = t - (t / NSLOT) * NSLOT;
    vn = inside(k);
    const float* xp = X + (size_t)(vn ? Pc + a.di[k] * a.w + a.dj[k] : Pc) * C_IN + s * KS + kh * (KS / 2);
#pragma unroll
    for (int st = 0; st < ST; ++st) xn[st] = *reinterpret_cast<const cp_f4*>(xp + 4 * st);
    const float* wp = Wimg + ((size_t)k * NSLOT + s) * SLOT_F + tid * 4;
#pragma unroll
    for (int p = 0; p < W_ITERS; ++p) wn[p] = *reinterpret_cast<const cp_f4*>(wp + p * CP_NT * 4);
  };
  auto put = [&](int buf) {   // the loaded slot becomes the current one: weights to LDS, the B operand selected (outside the map: exactly 0)
#pragma unroll
    for (int p = 0; p < W_ITERS; ++p) *reinterpret_cast<cp_f4*>(&cp_w[buf][(p * CP_NT + tid) * 4]) = wn[p];
#pragma unroll
    for (int st = 0; st < ST; ++st) xc[st] = vn ? xn[st] : cp_f4{0.f, 0.f, 0.f, 0.f};
  };

  x3_f16 tot[NM], acc[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[m][r] = 0.f;

  load(0);
  put(0);
  __syncthreads();

  const int fw = (kh * C_OUT + li) * 4;   // A fragment of step st, tile m: cp_w[buf][fw + (st 2 C_OUT + 32 m) 4]
  int t = 0;
#pragma unroll 1
  for (int k = kbeg; k < kend; ++k) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
#pragma unroll 1
    for (int s = 0; s < NSLOT; ++s, ++t) {
      load(t + 1 < T ? t + 1 : t);          // straight-line code: behind the last slot a harmless re-read
      __builtin_amdgcn_sched_barrier(0);    // the loads are issued HERE, a slot of MFMAs in front of their use
      const float* ws = &cp_w[t & 1][fw];
#pragma unroll
      for (int st = 0; st < ST; ++st) {
        cp_f4 af[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) af[m] = *reinterpret_cast<const cp_f4*>(ws + (st * 2 * C_OUT + m * 32) * 4);
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].x, xc[st].x, acc[m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].y, xc[st].y, acc[m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].z, xc[st].z, acc[m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m].w, xc[st].w, acc[m], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);    // (the scheduler would otherwise hoist the stores to the loads, and wait for them there)
      put((t + 1) & 1);                     // buffer (t + 1) & 1 was last read in slot t - 1, in front of that slot's barrier
      __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) tot[m] = tot[m] + acc[m];
  }

  // ---- epilogue: the bias vectors of the phase's blocks whose coarse pixel is inside the map, ascending; accumulator register r of tile m = output channel
  // 32 m + (r & 3) + 8 (r >> 2) + 4 kh of this lane's pixel
#pragma unroll 1
  for (int k = kbeg; k < kend; ++k) {
    const bool v = inside(k);
    const float* bp = bc + (size_t)k * C_OUT + 4 * kh;
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        cp_f4 b = *reinterpret_cast<const cp_f4*>(bp + m * 32 + 8 * g4);
        if (!v) b = cp_f4{0.f, 0.f, 0.f, 0.f};
        tot[m][4 * g4] += b.x; tot[m][4 * g4 + 1] += b.y; tot[m][4 * g4 + 2] += b.z; tot[m][4 * g4 + 3] += b.w;
      }
  }
#pragma unroll
  for (int m = 0; m < NM; ++m) asm volatile("" : "+v"(tot[m]));   // every load is consumed in front of the masked stores
  const size_t opix = ((size_t)bi * (F * a.h) + F * i + a.pa[ph]) * (size_t)(F * a.w) + F * j + a.pb[ph];
  if (live) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<cp_f4*>(out + opix * C_OUT + m * 32 + 8 * g4 + 4 * kh) = cp_f4{tot[m][4 * g4], tot[m][4 * g4 + 1], tot[m][4 * g4 + 2], tot[m][4 * g4 + 3]};
  }
}

// ---- weights: composed float32 [block][Cout][Cin] -> [block][slot][st][k-half 2][oc Cout][4 floats]; one thread = one 16-byte item
__global__ __launch_bounds__(256) void k_conv_poly_pack(const float* __restrict__ Wc, int Cout, int Cin, int nblk, float4* __restrict__ img) {
  const int ks = cp_ks(Cin), st_n = ks / 8;
  const int total = nblk * (Cin / ks) * st_n * 2 * Cout;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int oc = t % Cout, khalf = (t / Cout) & 1, st = (t / (2 * Cout)) % st_n, bs = t / (2 * Cout * st_n);   // bs = block * slots + slot
  const int k = bs / (Cin / ks), s = bs - k * (Cin / ks);
  const float* w = Wc + ((size_t)k * Cout + oc) * Cin + s * ks + khalf * (ks / 2) + 4 * st;
  img[t] = make_float4(w[0], w[1], w[2], w[3]);
}

static bool cp_built(int Cin, int Cout, int f) {
  return (Cin == 96 && Cout == 128 && f == 4) || (Cin == 192 && Cout == 128 && f == 2) || (Cin == 48 && Cout == 64 && f == 4) || (Cin == 96 && Cout == 64 && f == 2);
}
int vd_neck_poly_blocks(int f) { return (f == 2 || f == 4) ? cp_nblk(f) : -1; }
long long vd_neck_poly_weight_bytes(int Cin, int Cout, int f) {
  if (!cp_built(Cin, Cout, f)) return -1;
  return (long long)cp_nblk(f) * Cout * Cin * 4;
}
bool vd_launch_neck_poly_pack(hipStream_t s, const float* Wc, int Cin, int Cout, int f, void* img) {
  if (!cp_built(Cin, Cout, f) || (reinterpret_cast<uintptr_t>(img) & 15) || (reinterpret_cast<uintptr_t>(Wc) & 15)) return false;
  const int total = cp_nblk(f) * Cin * Cout / 4;
  hipLaunchKernelGGL(k_conv_poly_pack, dim3((total + 255) / 256), dim3(256), 0, s, Wc, Cout, Cin, cp_nblk(f), reinterpret_cast<float4*>(img));
  return true;
}
bool vd_neck_poly_shape_ok(int B, int h, int w, int Cin, int Cout, int f) {
  if (!cp_built(Cin, Cout, f) || B < 1 || h < 1 || w < 1) return false;
  const long long npix = (long long)B * h * w;
  if (npix * Cin >= (1ll << 31) || npix * f * f >= (1ll << 31)) return false;   // 32-bit pixel indices; the element offsets are 64-bit
  return true;
}

// the block table: phases (pa, pb) row-major, offsets di ascending then dj ascending; the workgroups' phases in descending cost (the long ones start first)
static void cp_table(int f, vd_cp_args& a, int& nph) {
  int first[CP_MAXPH], count[CP_MAXPH], k = 0;
  for (int pa = 0; pa < f; ++pa)
    for (int pb = 0; pb < f; ++pb) {
      first[pa * f + pb] = k;
      for (int di = (pa == 0 ? -1 : 0); di <= (pa == f - 1 ? 1 : 0); ++di)
        for (int dj = (pb == 0 ? -1 : 0); dj <= (pb == f - 1 ? 1 : 0); ++dj, ++k) { a.di[k] = di; a.dj[k] = dj; }
      count[pa * f + pb] = k - first[pa * f + pb];
    }
  nph = 0;
  for (int c = 4; c >= 1; --c)
    for (int p = 0; p < f * f; ++p)
      if (count[p] == c) { a.kbeg[nph] = first[p]; a.kend[nph] = first[p] + c; a.pa[nph] = (p / f); a.pb[nph] = (p % f); ++nph; }
}

bool vd_launch_neck_poly_conv_f32(hipStream_t s, const float* x, int B, int h, int w, int Cin, const void* wimg, const float* bc, int Cout, int f, float* out) {
  if (!vd_neck_poly_shape_ok(B, h, w, Cin, Cout, f)) return false;
  vd_cp_args a = {};
  a.h = h; a.w = w; a.npix = B * h * w;
  int nph = 0;
  cp_table(f, a, nph);
  const dim3 grid((unsigned)((a.npix + CP_PIX - 1) / CP_PIX), (unsigned)nph, 1);
  const float* wi = reinterpret_cast<const float*>(wimg);
  if (Cin == 96 && Cout == 128) hipLaunchKernelGGL((k_conv_poly_f32<96, 128, 4>), grid, dim3(CP_NT), 0, s, x, wi, bc, out, a);
  else if (Cin == 192) hipLaunchKernelGGL((k_conv_poly_f32<192, 128, 2>), grid, dim3(CP_NT), 0, s, x, wi, bc, out, a);
  else if (Cin == 48) hipLaunchKernelGGL((k_conv_poly_f32<48, 64, 4>), grid, dim3(CP_NT), 0, s, x, wi, bc, out, a);
  else hipLaunchKernelGGL((k_conv_poly_f32<96, 64, 2>), grid, dim3(CP_NT), 0, s, x, wi, bc, out, a);
  return true;
}
