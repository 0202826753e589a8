// vd3d_attn.hip -- softmax(Q K^T * scale) V of the depth network's transformer blocks (boundary B3, core/render_depth.py:1106-1119: float32 through the
// Hugging Face pipeline) with BOTH matrix products as split-bf16 MFMA work -- the attention half of the opt-in `gemm="bf16x3"` mode (round 6; gfx950's
// float32-input MFMA runs at 1/16 of the bf16 rate) -- and, further down, k_attn_f32: the same attention in exact float32, the default mode's (it replaced
// PyTorch's scaled_dot_product_attention = AOTriton's float32 kernel, 99.5 TFLOP/s, with 113.5 at the 4K DA-V2-Base shape).  Same arithmetic idea as vd3d_gemm.hip: every float32 operand (Q, K, V and the probabilities P) is split EXACTLY into three bf16
// terms, six of the nine term products go through v_mfma_f32_32x32x16_bf16 with float32 accumulation (the dropped ones are <= 2^-23 of a product);
// the softmax itself is float32 (running maximum / sum, exp2 of the pre-scaled logits by v_exp_f32).
//
// Two kernels per call:
//   k_attn_x3_prep   qkv [B][T][3][H][64] float32 (the fused QKV linear's output) -> three split + packed images, rows past T zero:
//       Q  [b h][q block 32][k-step 4][term 3][k-half 2][q 32][8 bf16]       (B-operand fragments, read once per wave straight into registers)
//       K  [b h][kv tile 64][k-step 4][term 3][k-half 2][kv 64][8 bf16]      (A-operand fragments of S^T = K Q^T; 24 KB per tile, contiguous)
//       V^T[b h][kv tile 64][k-step 4][term 3][k-half 2][d 64][8 bf16]       (A-operand fragments of O^T = V^T P^T; the 16 kv slots of a k-step are
//                                                                             PERMUTED to where the S^T accumulator leaves them, see below)
//   k_attn_bf16x3    one workgroup = 256 queries of one (batch, head): 8 waves x 32 queries, 512 threads, two waves per SIMD.  Per 64-row KV tile
//       (LDS-DMA into a ring of three 48 KB stages, K three and V^T two tiles ahead, counted vmcnt + raw s_barrier; S^T of tile it + 1 is issued beside the softmax of tile it):
//         S^T[kv 64][q 32] = K Q^T          2 M tiles x 4 k-steps x 6 products = 48 MFMAs.  TRANSPOSED on purpose: the accumulator layout (column =
//                                            lane & 31 = the query, rows = kv in registers) makes every softmax reduction an IN-LANE loop over 32
//                                            registers plus one exchange with lane ^ 32, and the per-query scalars (max, sum, rescale) per-lane values;
//         online softmax                     z = s * (scale * log2 e), m' = max(m, max z), p = exp2(z - m'), l = l * exp2(m - m') + sum p, O *= exp2(m - m')
//         O^T[d 64][q 32] += V^T P^T         P^T as the B operand comes straight out of the S^T accumulator registers: k-step j of M tile m uses registers
//                                            8 j .. 8 j + 7, i.e. kv = 32 m + (e & 3) + 8 (2 j + (e >> 2)) + 4 (lane >> 5) for element e -- the order the
//                                            V^T image is packed in.  No LDS round trip, no cross-lane movement.  2 x 4 x 6 = 48 MFMAs.
//       Epilogue: O^T / l through LDS (272-byte rows: conflict-free 16-byte writes per query) to out[b][t][h][64] in 256-byte row segments.
// Work per tile and wave: 96 MFMAs (3 072 cycles of a SIMD's matrix pipe) against ~500 VALU instructions (softmax + the exact split of 32
// probabilities per lane).  A CU ingests 48 KB per tile = 8 bytes per matrix-pipe cycle: under its ~12 B / cycle vector-memory limit (with 128 queries
// per workgroup it would be 16: the reason for the 8-wave workgroup).
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include "vd3d_x3.h"

#include <mutex>

#define AT_D 64
#define AT_BQ 256
#define AT_BK 64
#define AT_NT 512
// MODE 0 = bf16x3 (three exact bf16 terms, six products), MODE 1 = fp16x2 (two fp16 terms = 22 bits, three products: half the matrix work; q, k, v are scaled
// by 2^4 and the probabilities by 2^10 before their split -- exact -- so that the second terms stay normal fp16 numbers; vd3d_gemm.hip, include/vd3d.h)
#define AT_NTERM(MODE) ((MODE) == 0 ? 3 : 2)
#define AT_TILE(MODE) (4 * AT_NTERM(MODE) * 2 * 64 * 16)   // one K or V^T tile image: 24 576 / 16 384 bytes
#define AT_STAGE(MODE) (2 * AT_TILE(MODE))                 // K + V^T: 49 152 / 32 768
#define AT_NSTAGE 3
#define AT_LDS(MODE) (AT_NSTAGE * AT_STAGE(MODE))          // 147 456 / 98 304
#define AT_QBLK(MODE) (4 * AT_NTERM(MODE) * 2 * 32)        // uint4 per 32-query block of the Q image
#define AT_QKV_SCALE 16.0f                                 // fp16x2: q, k, v times 2^4 ...
#define AT_P_SCALE 1024.0f                                 // ... and p times 2^10 before the split
#define AT_OP 272                             // epilogue: bytes per query row in LDS (256 + 16)

struct vd_at_args {
  int B, H, T;
  int nq32, nkv, nqb;        // 32-query blocks, 64-row KV tiles, 256-query workgroups per (b, h)
  float c;                   // scale * log2(e)
};

// ---- prep: one thread = 8 consecutive elements of one fragment chunk.  which 0 / 1 (Q, K): 8 consecutive d of one token; which 2 (V^T): the 8 kv slots
// of one (k-step, k-half) at one d.
template <int MODE>
__global__ __launch_bounds__(256) void k_attn_x3_prep(const float* __restrict__ qkv, vd_at_args a, uint4* __restrict__ Qimg, uint4* __restrict__ Kimg,
                                                      uint4* __restrict__ Vimg) {
  constexpr int NTERM = AT_NTERM(MODE);
  const int which = blockIdx.z, bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int t_id = blockIdx.x * 256 + threadIdx.x;
  const size_t tok_stride = (size_t)3 * a.H * AT_D;
  float v[8];
  uint4* dst;
  if (which < 2) {
    const int rows = which == 0 ? a.nq32 * 32 : a.nkv * 64;
    const int t = t_id >> 3, c = t_id & 7;       // token, chunk of 8 d
    if (t >= rows) return;
    if (t < a.T) {
      const float* src = qkv + ((size_t)b * a.T + t) * tok_stride + (size_t)which * a.H * AT_D + h * AT_D + c * 8;
      const float4 lo = *reinterpret_cast<const float4*>(src), hi = *reinterpret_cast<const float4*>(src + 4);
      v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
    const int ks = c >> 1, kh = c & 1;
    if (which == 0) dst = Qimg + ((size_t)bh * a.nq32 + (t >> 5)) * AT_QBLK(MODE) + (size_t)((ks * NTERM) * 2 + kh) * 32 + (t & 31);
    else dst = Kimg + ((size_t)bh * a.nkv + (t >> 6)) * (AT_TILE(MODE) / 16) + (size_t)((ks * NTERM) * 2 + kh) * 64 + (t & 63);
    x3_s8 o[NTERM];
    x3_split8_m<MODE>(v, AT_QKV_SCALE, o);
    const int ts = which == 0 ? 2 * 32 : 2 * 64;   // term stride in uint4
#pragma unroll
    for (int t3 = 0; t3 < NTERM; ++t3) dst[(size_t)t3 * ts] = __builtin_bit_cast(uint4, o[t3]);
  } else {
    // V^T: thread = (kv tile, k-step, k-half, d); d fastest so that a wave reads 64 consecutive floats of a token row
    const int d = t_id & 63, kh = (t_id >> 6) & 1, ks = (t_id >> 7) & 3, tile = t_id >> 9;
    if (tile >= a.nkv) return;
    const int m = ks >> 1, j = ks & 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kv = tile * 64 + 32 * m + (e & 3) + 8 * (2 * j + (e >> 2)) + 4 * kh;
      v[e] = kv < a.T ? qkv[((size_t)b * a.T + kv) * tok_stride + (size_t)2 * a.H * AT_D + h * AT_D + d] : 0.f;
    }
    x3_s8 o[NTERM];
    x3_split8_m<MODE>(v, AT_QKV_SCALE, o);
    dst = Vimg + ((size_t)bh * a.nkv + tile) * (AT_TILE(MODE) / 16) + (size_t)((ks * NTERM) * 2 + kh) * 64 + d;
#pragma unroll
    for (int t3 = 0; t3 < NTERM; ++t3) dst[(size_t)t3 * 128] = __builtin_bit_cast(uint4, o[t3]);
  }
}

// six products (small first: x3 w1, x2 w2, x1 w3, x2 w1, x1 w2, x1 w1) into TWO accumulators that share the B operand, alternating: dependent MFMAs 64 cycles apart
#define AT_MM1(ACC0, AF0, ACC1, AF1, BF, ta, tb)                                               \
  ACC0 = x3_mfma<MODE>(AF0[ta], BF[tb], ACC0);                                                 \
  ACC1 = x3_mfma<MODE>(AF1[ta], BF[tb], ACC1);
#define AT_MM6(ACC0, AF0, ACC1, AF1, BF)                                                       \
  if (MODE == 0) { AT_MM1(ACC0, AF0, ACC1, AF1, BF, NTERM - 1, 0) AT_MM1(ACC0, AF0, ACC1, AF1, BF, 1, 1) AT_MM1(ACC0, AF0, ACC1, AF1, BF, 0, NTERM - 1) }                               \
  AT_MM1(ACC0, AF0, ACC1, AF1, BF, 1, 0) AT_MM1(ACC0, AF0, ACC1, AF1, BF, 0, 1) AT_MM1(ACC0, AF0, ACC1, AF1, BF, 0, 0)

template <int MODE>
__global__ __launch_bounds__(AT_NT) void k_attn_bf16x3(const uint4* __restrict__ Qimg, const uint4* __restrict__ Kimg, const uint4* __restrict__ Vimg,
                                                       float* __restrict__ out, vd_at_args a) {
  constexpr int NTERM = AT_NTERM(MODE), TILE = AT_TILE(MODE), STAGE = AT_STAGE(MODE), NP = TILE / (AT_NT * 16);   // DMA instructions per thread and operand tile: 3 / 2
  extern __shared__ __attribute__((aligned(16))) uint8_t at_lds[];   // the only LDS object (see vd3d_gemm.hip)
  // workgroups of one (b, h) share its K / V^T images: keep them on one XCD (workgroup id mod 8; speed only)
  int bh, qb;
  {
    const int wg = blockIdx.x, x = wg & 7, idx = wg >> 3;
    const int g = idx / a.nqb;
    qb = idx - g * a.nqb;
    bh = g * 8 + x;
    if (bh >= a.B * a.H) return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kh = lane >> 5;
  const int q0 = qb * AT_BQ + wave * 32;                 // first query of this wave
  const int wave_base = (tid & ~63) * 16;

  // Q fragments of the wave's 32 queries (zero rows past T: the image is padded to whole 32-query blocks; a wave past the last block reads block nq32 - 1 and
  // stores nothing)
  x3_s8 qf[4][NTERM];
  {
    const int blk = min(q0 >> 5, a.nq32 - 1);
    const uint4* qp = Qimg + ((size_t)bh * a.nq32 + blk) * AT_QBLK(MODE) + kh * 32 + li;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int t = 0; t < NTERM; ++t) qf[ks][t] = __builtin_bit_cast(x3_s8, qp[(ks * NTERM + t) * 64]);
  }
  const uint4* kimg = Kimg + (size_t)bh * a.nkv * (TILE / 16) + tid;
  const uint4* vimg = Vimg + (size_t)bh * a.nkv * (TILE / 16) + tid;
  // one DMA instruction of a tile: pieces 0 .. 2 = K, 3 .. 5 = V^T (512 x 16 bytes each; fp16x2 tiles are two pieces: piece 2 / 5 does nothing there)
  auto dma = [&](int tile, int buf, int piece) {
    const int op = piece / 3, pp = piece - 3 * op;
    if (pp >= NP) return;
    const uint4* src = (op == 0 ? kimg : vimg) + (size_t)tile * (TILE / 16) + pp * AT_NT;
    uint8_t* dst = at_lds + buf * STAGE + op * TILE + pp * (AT_NT * 16) + wave_base;
    __builtin_amdgcn_global_load_lds((x3_glb_vp)src, (x3_lds_vp)dst, 16, 0, 0);
  };

  x3_f16 oacc[2];
#pragma unroll
  for (int dm = 0; dm < 2; ++dm)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dm][r] = 0.f;
  float m_run = -INFINITY, l_half = 0.f;

  // Software pipeline INSIDE a wave: the S^T MFMAs of tile it + 1 are issued in the same straight-line region as the softmax VALU work of tile it (independent
  // data: hipcc interleaves them, sched_group_barrier says how), then P V of tile it with the split of the next k-step's probabilities between its MFMAs.  A
  // wave that alternated MFMA phases and VALU phases left the matrix pipe idle whenever both waves of a SIMD were in a VALU phase -- and the per-tile barrier
  // keeps them in step (measured: 1.89 ms per DA-V2-Base call at 4K = 0.93 PFLOP/s of MFMA work).
  // So K (t) is read in iteration t - 1 and V^T (t) in iteration t.  Stage s of the ring holds tile t with t % 3 == s; iteration it issues the DMA of K (it + 3)
  // [its stage's K was last read in iteration it - 1] and of V^T (it + 2) [its stage's V^T was last read in iteration it - 1]; the wait at the end lets the six
  // instructions just issued stay in flight and so guarantees K (it + 2) and V^T (it + 1), issued one iteration earlier.
  const int last_tile = a.nkv - 1;
  auto tile_c = [&](int t) { return t < last_tile ? t : last_tile; };   // behind the last tile: re-fetch it into a stage nobody reads again (straight-line code)
#pragma unroll
  for (int p = 0; p < 6; ++p) dma(0, 0, p);                 // K (0), V^T (0)
#pragma unroll
  for (int p = 0; p < 3; ++p) dma(tile_c(1), 1, p);         // K (1)
#pragma unroll
  for (int p = 3; p < 6; ++p) dma(tile_c(1), 1, p);         // V^T (1)
#pragma unroll
  for (int p = 0; p < 3; ++p) dma(tile_c(2), 2, p);         // K (2)
  if (NP == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // K (0), V^T (0), K (1) landed; V^T (1), K (2) in flight
  __builtin_amdgcn_s_barrier();

  const int frag_off = (kh * 64 + li) * 16;     // + ((ks * 3 + t) * 2) * 1024 + m * 512
  // one k-step (16 of the 64 head dimensions) of S^T for both 32-row M tiles: 6 fragment reads, 12 MFMAs
  auto st_step = [&](const uint8_t* sk, int ks, x3_f16 (&sa)[2]) {
    x3_s8 kf[2][NTERM];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int t = 0; t < NTERM; ++t) kf[m][t] = *reinterpret_cast<const x3_s8*>(sk + frag_off + ((ks * NTERM + t) * 2) * 1024 + m * 512);
    AT_MM6(sa[0], kf[0], sa[1], kf[1], qf[ks])
  };
  // hint for one pinned chunk: 12 x (one MFMA = 32 cycles of the SIMD's matrix pipe, then up to n VALU), the fragment reads first
#define AT_CHUNK_HINT(n)                                           \
  __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);               \
  _Pragma("unroll") for (int i_ = 0; i_ < 12; ++i_) {              \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);             \
    __builtin_amdgcn_sched_group_barrier(0x002, n, 0);             \
  }                                                                \
  __builtin_amdgcn_sched_barrier(0);

  x3_f16 sacc[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[m][r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) st_step(at_lds, ks, sacc);   // S^T (0)
  // the first iteration's DMA of K (3) overwrites K (0): every wave's reads of it have returned first (found the hard way: one shape in twenty, under load)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  int cur = 0;
  for (int it = 0; it < a.nkv; ++it) {
    const int s1 = cur == 2 ? 0 : cur + 1, s2 = cur >= 1 ? cur - 1 : 2;   // stages of tiles it + 1 and it + 2 (= it - 1)
    const uint8_t* sk1 = at_lds + s1 * STAGE;
    const uint8_t* sv = at_lds + cur * STAGE + TILE;
    // ---- tile it: logits -> z (pre-scaled; rows past T masked in the last tile: a uniform branch off the hot path)
    float z[2][16];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) z[m][r] = sacc[m][r] * a.c;
    if ((it + 1) * AT_BK > a.T) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (it * AT_BK + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * kh >= a.T) z[m][r] = -INFINITY;
    }
    // ---- region A: S^T (it + 1) on the matrix pipe || softmax (it) on the VALU, in four pinned chunks of 12 MFMAs
    x3_f16 sn[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) sn[m][r] = 0.f;
    // chunk 0: running maximum
    dma(tile_c(it + 3), cur, 0);                       // K (it + 3) -> this tile's stage (its K was consumed in iteration it - 1)
    __builtin_amdgcn_sched_barrier(0);
    st_step(sk1, 0, sn);
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, z[m][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    AT_CHUNK_HINT(2)
    // chunks 1, 2: the exponentials of one M tile each
    float ps = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      dma(tile_c(it + 3), cur, 1 + m);
      __builtin_amdgcn_sched_barrier(0);
      st_step(sk1, 1 + m, sn);
#pragma unroll
      for (int r = 0; r < 16; ++r) { z[m][r] = __builtin_amdgcn_exp2f(z[m][r] - m_new); ps += z[m][r]; }
      AT_CHUNK_HINT(4)
    }
    // chunk 3: rescale O, split the first k-step's probabilities
    dma(tile_c(it + 2), s2, 3);                        // V^T (it + 2) -> the stage of tile it - 1 (its V^T was consumed in iteration it - 1)
    __builtin_amdgcn_sched_barrier(0);
    st_step(sk1, 3, sn);
    l_half = l_half * alpha + ps;
#pragma unroll
    for (int dm = 0; dm < 2; ++dm)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dm][r] *= alpha;
    x3_s8 pf[2][NTERM];
    x3_split8_m<MODE>(&z[0][0], AT_P_SCALE, pf[0]);
    AT_CHUNK_HINT(7)
    // ---- region B: O^T += V^T P^T (tile it); the split of k-step ks + 1 rides on the MFMAs of k-step ks
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks < 2) { dma(tile_c(it + 2), s2, 4 + ks); __builtin_amdgcn_sched_barrier(0); }
      if (ks < 3) x3_split8_m<MODE>(&z[(ks + 1) >> 1][8 * ((ks + 1) & 1)], AT_P_SCALE, pf[(ks + 1) & 1]);
      x3_s8 vf[2][NTERM];
#pragma unroll
      for (int dm = 0; dm < 2; ++dm)
#pragma unroll
        for (int t = 0; t < NTERM; ++t) vf[dm][t] = *reinterpret_cast<const x3_s8*>(sv + frag_off + ((ks * NTERM + t) * 2) * 1024 + dm * 512);
      AT_MM6(oacc[0], vf[0], oacc[1], vf[1], pf[ks & 1])
      AT_CHUNK_HINT(4)
    }
    // K (it + 2) and V^T (it + 1) have landed for everyone (a wave's own DMAs of them are older than the six instructions it just issued), and this wave's LDS
    // reads of the stages it used have returned, before anybody overwrites them
    if (NP == 3) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int m = 0; m < 2; ++m) sacc[m] = sn[m];
    cur = s1;
  }
#undef AT_CHUNK_HINT
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-fetches of the last iterations have landed ...
  __builtin_amdgcn_s_barrier();                        // ... everybody's, before the epilogue re-uses the ring

  // ---- epilogue: O^T / l -> LDS [q 32 per wave][d 64] with 272-byte rows -> out[b][t][h][d]
  const float l_tot = l_half + __shfl_xor(l_half, 32, 64);
  const float inv = MODE == 1 ? 1.0f / (l_tot * (AT_P_SCALE * AT_QKV_SCALE)) : 1.0f / l_tot;   // fp16x2: O accumulated (2^10 p)(2^4 v)
  uint8_t* ow = at_lds + wave * (32 * AT_OP);
#pragma unroll
  for (int dm = 0; dm < 2; ++dm)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 v4 = {oacc[dm][4 * g] * inv, oacc[dm][4 * g + 1] * inv, oacc[dm][4 * g + 2] * inv, oacc[dm][4 * g + 3] * inv};
      *reinterpret_cast<float4*>(ow + li * AT_OP + (32 * dm + 8 * g + 4 * kh) * 4) = v4;
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // own wave's rows only: no barrier needed (wave-private region; LDS ops of a wave complete in order)
  const int b = bh / a.H, h = bh - b * a.H;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = i * 4 + (lane >> 4), c4 = lane & 15;   // 16 lanes x 16 bytes = one query's 256 bytes
    const int q = q0 + row;
    const float4 v4 = *reinterpret_cast<const float4*>(ow + row * AT_OP + c4 * 16);
    if (q < a.T) *reinterpret_cast<float4*>(out + (((size_t)b * a.T + q) * a.H + h) * AT_D + c4 * 4) = v4;
  }
}

// ---- exact float32: k_attn_f32 (the default mode's attention) ------------------------------------------------------------------------------------------
// The same S^T / P^T-from-the-accumulator layout on v_mfma_f32_32x32x2_f32 (A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31], one float32
// per lane; a k-ordered fmaf chain, 64 cycles issue and dependent latency), with no split and no prep pass: Q comes straight from qkv into registers, K and V
// rows (256 bytes per token and head) stream from qkv into an LDS ring by LDS-DMA.
//   S^T[kv 32][q 32] (M tile m)   k-step s = 0 .. 31 takes d = 32 (lane >> 5) + s: a lane's 32 q values are one 128-byte run of its query row (eight 16-byte
//                                  loads, scaled by scale * log2 e once) and its K values four 16-byte LDS reads per M tile.  2 x 32 = 64 MFMAs per 64-row tile.
//   O^T[d 32][q 32] (tile dm)      accumulator register r of M tile m is one K = 2 step: P^T as the B operand straight from the S^T registers, lane half k
//                                  holding kv = 32 m + (r & 3) + 8 (r >> 2) + 4 k; the A operand is V^T with row i = lane & 31 taken as d = 2 i + dm, so one
//                                  ds_read_b64 of V[kv][2 i .. 2 i + 1] feeds both d tiles.  2 x 32 = 64 MFMAs per tile.  In the accumulator, registers
//                                  4 g .. 4 g + 3 of both tiles are d = 16 g + 8 k .. + 7 of one query: the epilogue stores 32 contiguous bytes per lane and g.
// LDS: a ring of three stages (K 16 KB, V 16 KB each), tile it + 2 issued at the top of iteration it into the stage tile it - 1 left (the barrier at the end
// of iteration it - 1 follows every wave's reads of it).  K is XOR-swizzled (16-byte chunk c of row r at chunk c ^ (r & 15): the DMA picks each lane's source
// chunk, the LDS image stays lane-linear) so that the 16-lane groups of ds_read_b128 see 16 distinct chunks; V is linear (a ds_read_b64 of 32 lanes reads one
// whole 256-byte row).  Every DMA source row is clamped to T - 1: no zero-padded image, nothing read past the tensor, logits of rows past T are finite before
// they are masked to -inf (p = 0 exactly).  O is rescaled only when some lane's running maximum grew (alpha = exp2(0) = 1 exactly for the others).
// What the tile loop issues per wave and 64-row tile (profiles/r23_attn_f32_lean.md): 128 MFMAs (8 192 matrix-pipe cycles) and ~131 VALU instructions -- 32
// v_sub, 32 v_exp, 33 v_add, 16 v_max3 + 3 v_max, 4 for the cross-half maximum (v_permlane32_swap) and the rescale test, and 11 of addresses (3 for the
// tile's DMA, 8 bases of the paired V reads), down from 63 of addresses in the 4-wave form: the DMA sources are a scalar base per tile and pass plus a per-lane offset computed once, and the loop is
// unrolled over the ring so that every LDS read is a loop-invariant register plus an immediate.  On gfx950 float32-input MFMA and the VALU share the FP32
// ALUs: their times add wherever the instructions are scheduled, so issuing the next tile's S^T under the softmax is NOT an open lever here (two attempts
// measured nothing); only fewer vector instructions per tile are.
// A last tile with at most 32 live rows (T mod 64 in 1 .. 32) runs outside the loop with its second 32-row M tile left out of both products.  For S^T this is
// exact on every input (those 16 logits are masked to -inf either way).  For P V it drops 32 MFMAs that add v * 0 to every accumulator, which changes a result
// in two cases only, neither reachable from finite data: an accumulator that is exactly -0 (the + 0 made it +0) and a non-finite V in the clamped row T - 1
// (inf * 0 made it NaN).
#define AF_TILE (AT_BK * AT_D * 4)   // 16 384 bytes: 64 rows x 256
#define AF_STAGE (2 * AF_TILE)       // K + V
#define AF_LDS(NS) ((NS) * AF_STAGE)   // 98 304 (8 waves, three stages) / 65 536 (4 waves, two stages)
// Two forms of one kernel, k_attn_f32<NW, NS>: NW waves (32 NW queries) per workgroup, a ring of NS stages.
//   <8, 3>  256 queries, 96 KB: one workgroup per CU, two waves per SIMD held in step by one barrier per tile.
//   <4, 2>  128 queries, 64 KB, __launch_bounds__(256, 2): TWO workgroups per CU, again two waves per SIMD but with independent barriers (the two are not forced
//           into the softmax at the same moment), twice as many equal workgroups (the last, partly filled round of the grid leaves each SIMD's matrix pipe to one
//           wave instead of idling half the CUs) and padding waves that skip their matrix work (below).  Tile it + 1 is issued at the top of iteration it into
//           the stage tile it - 1 left and waited for (vmcnt(0)) in front of the barrier that ends the iteration: a tile has > 8 000 matrix-pipe cycles to
//           land, one tile ahead is enough.  K/V are staged per 128 queries: ~4 bytes per matrix-pipe cycle and CU, a third of the ~12 B / cycle limit.
// Per query both forms run the same operations in the same order (tiles ascending, the two S^T chains, masking, maximum, rescale, sum order, P V chain, division):
// their results are bit-identical (tests/test_hip_attention_f32_forms.py).
static_assert(2 * AF_LDS(2) <= 160 * 1024, "two 4-wave workgroups per CU");
static_assert(AF_LDS(2) == 65536 && AF_LDS(3) == 98304, "the rings' dynamic LDS; the two-stage ring ends at byte 65 535, the reach of a DS instruction's offset field");
// The two matrix products of one tile, each reading its stage of the ring through a restrict pointer: inlined, the LDS reads carry alias-scope information
// (one scope per product, kept when the compiler pairs reads), and the compiler's wait-count pass then does not put a conservative vmcnt(0) behind every
// LDS-DMA in front of them -- the ring is ordered by the kernel's own counted waits and barriers.
// Both take the ring stage as an argument that is a constant in every copy of the unrolled tile loop, and the lane's part of the address from loop-invariant
// registers: a K read is one register plus an immediate (the paired V reads take one base per four rows).
// NM = 2: the whole 64-row tile.  NM = 1: its first 32-row M tile only -- a last tile whose rows 32 .. 63 are all past T (the header above says what that leaves out).
// S^T[m] = K Q^T for the 32-row M tiles m = 0, 1 (q pre-scaled); K row r at 256 r of its tile, 16-byte chunk c at position c ^ (r & 15):
// kp[g] = at_lds + 256 li + (((8 kh + g) << 4) ^ ((li & 15) << 4)), the lane's row and swizzled chunk of k-steps 4 g .. 4 g + 3 in stage 0.  NM = 1 leaves
// S^T[1] at -inf.  af_st_g is the four k-steps of one g (one restrict pointer, one alias scope each), af_st the product.
template <int N> struct af_ic { static constexpr int value = N; };
template <int NM, int G>
VD_DEV void af_st_g(const uint8_t* __restrict__ kp, int stage, const float (&qf)[32], x3_f16 (&s)[2]) {
  float4 kf[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) kf[m] = *reinterpret_cast<const float4*>(kp + stage * AF_STAGE + 32 * 256 * m);
#pragma unroll
  for (int m = 0; m < NM; ++m) s[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[m].x, qf[4 * G], s[m], 0, 0, 0);
#pragma unroll
  for (int m = 0; m < NM; ++m) s[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[m].y, qf[4 * G + 1], s[m], 0, 0, 0);
#pragma unroll
  for (int m = 0; m < NM; ++m) s[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[m].z, qf[4 * G + 2], s[m], 0, 0, 0);
#pragma unroll
  for (int m = 0; m < NM; ++m) s[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[m].w, qf[4 * G + 3], s[m], 0, 0, 0);
}
template <int NM>
VD_DEV void af_st(const uint8_t* const (&kp)[8], int stage, const float (&qf)[32], x3_f16 (&s)[2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[m][r] = m < NM ? 0.f : -INFINITY;
  af_st_g<NM, 0>(kp[0], stage, qf, s); af_st_g<NM, 1>(kp[1], stage, qf, s); af_st_g<NM, 2>(kp[2], stage, qf, s); af_st_g<NM, 3>(kp[3], stage, qf, s);
  af_st_g<NM, 4>(kp[4], stage, qf, s); af_st_g<NM, 5>(kp[5], stage, qf, s); af_st_g<NM, 6>(kp[6], stage, qf, s); af_st_g<NM, 7>(kp[7], stage, qf, s);
}
// O^T[dm] += V^T P^T: register r of M tile m is the K = 2 step of kv 32 m + (r & 3) + 8 (r >> 2) + 4 kh; V row kv at sv + 256 kv (linear), d = 2 li + dm:
// va = 1 024 kh + 8 li.  One call is one M tile (M = 0, then M = 1: the chain's order).
template <int M>
VD_DEV void af_pv(const uint8_t* __restrict__ sv, const x3_f16 (&p)[2], uint32_t va, x3_f16 (&oacc)[2]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float2 vv = *reinterpret_cast<const float2*>(sv + va + (32 * M + (r & 3) + 8 * (r >> 2)) * 256);
    oacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.x, p[M][r], oacc[0], 0, 0, 0);
    oacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.y, p[M][r], oacc[1], 0, 0, 0);
  }
}

template <int NW, int NS>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void k_attn_f32(const float* __restrict__ qkv, float* __restrict__ out, vd_at_args a) {
  static_assert((NW == 8 && NS == 3) || (NW == 4 && NS == 2), "built forms");
  constexpr int NP = 16 / NW;   // DMA passes per thread and operand tile: 1 024 sixteen-byte chunks over NW * 64 threads
  extern __shared__ __attribute__((aligned(16))) uint8_t at_lds[];
  int bh, qb;   // (b, h) grouped by XCD as in k_attn_bf16x3: the workgroups of one (b, h) read the same K / V rows (and are consecutive in dispatch order on their XCD)
  {
    const int wg = blockIdx.x, x = wg & 7, idx = wg >> 3;
    const int g = idx / a.nqb;
    qb = idx - g * a.nqb;
    bh = g * 8 + x;
    if (bh >= a.B * a.H) return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kh = lane >> 5;
  const int q0 = qb * (NW * 32) + wave * 32;
  // 4-wave form: a wave whose 32 queries are all past T (padding of the last workgroup) does its share of the DMA and reaches every barrier, and nothing else:
  // its SIMD's matrix pipe is left to the co-resident workgroup's wave.  Wave-uniform (q0 is).  The 8-wave form computes them as it always did.
  const bool live = NW == 8 || q0 < a.T;
  const int b = bh / a.H, h = bh - b * a.H;
  const size_t tok_stride = (size_t)3 * a.H * AT_D;
  const float* base = qkv + (size_t)b * a.T * tok_stride + h * AT_D;   // q of token t at base + t tok_stride, k at + H 64, v at + 2 H 64

  // one tile's DMA: thread tid fills LDS chunks tid + 64 NW p (p < NP) of the K and of the V image = rows tid / 16 + 4 NW p, chunk position tid & 15 (4 NW is a
  // multiple of 16: the K swizzle of a thread is the same in every pass)
  // A tile that lies inside T is fetched with no vector arithmetic: the lane's byte offsets inside a pass (row drow, its K and its V chunk; below 2^32: 31 token
  // rows of 768 H bytes, H < 2^16) are computed once, and each DMA's source is a wave-uniform 64-bit base (tile and pass, scalar arithmetic) plus that 32-bit
  // offset.  Only the tile that crosses T needs its rows clamped to T - 1 per lane: a uniform branch that the last tile alone takes.
  const int drow = tid >> 4, dpos = tid & 15, kchunk = dpos ^ (drow & 15);
  const uint32_t tok_bytes = 3u * 4u * AT_D * (uint32_t)a.H;
  const uint32_t koff = (uint32_t)drow * tok_bytes + (uint32_t)kchunk * 16u, voff = (uint32_t)drow * tok_bytes + (uint32_t)dpos * 16u;
  const uint64_t kbase = reinterpret_cast<uint64_t>(base + a.H * AT_D), vbase = reinterpret_cast<uint64_t>(base + 2 * a.H * AT_D);
  auto dma = [&](int tile, int stage) {
    uint8_t* dst = at_lds + stage * AF_STAGE + wave * 1024;
    if ((tile + 1) * AT_BK <= a.T) {
      // the empty asm statements pin the two parts where they are used -- the base in scalar registers, the 32-bit offset widened here and not once in front
      // of the loop -- so that the load is selected in its scalar-base + 32-bit-offset form instead of one 64-bit sum per lane and load
      uint32_t ko = koff, vo = voff;
      asm("" : "+v"(ko), "+v"(vo));
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const uint64_t row0 = (uint64_t)(tile * AT_BK + 4 * NW * p) * tok_bytes;
        uint64_t ks = kbase + row0, vs = vbase + row0;
        asm("" : "+s"(ks), "+s"(vs));
        __builtin_amdgcn_global_load_lds((x3_glb_vp)(ks + ko), (x3_lds_vp)(dst + p * (NW * 1024)), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((x3_glb_vp)(vs + vo), (x3_lds_vp)(dst + AF_TILE + p * (NW * 1024)), 16, 0, 0);
      }
    } else {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int tok = min(tile * AT_BK + drow + 4 * NW * p, a.T - 1);
        const float* src = base + (size_t)tok * tok_stride + a.H * AT_D;
        __builtin_amdgcn_global_load_lds((x3_glb_vp)(src + kchunk * 4), (x3_lds_vp)(dst + p * (NW * 1024)), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((x3_glb_vp)(src + a.H * AT_D + dpos * 4), (x3_lds_vp)(dst + AF_TILE + p * (NW * 1024)), 16, 0, 0);
      }
    }
  };
  // the lane's part of every LDS read address (af_st, af_pv)
  const uint8_t* kp[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) kp[g] = at_lds + (li * 256 + (((8 * kh + g) << 4) ^ ((li & 15) << 4)));
  const uint32_t va = (uint32_t)(kh * 1024 + li * 8);

  // Q of the wave's 32 queries (rows past T read row T - 1 and are never stored), pre-scaled by scale * log2 e
  float qf[32];
  if (live) {
    const float4* qp = reinterpret_cast<const float4*>(base + (size_t)min(q0 + li, a.T - 1) * tok_stride + 32 * kh);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const float4 v = qp[g];
      qf[4 * g] = v.x * a.c; qf[4 * g + 1] = v.y * a.c; qf[4 * g + 2] = v.z * a.c; qf[4 * g + 3] = v.w * a.c;
    }
  } else {
#pragma unroll
    for (int g = 0; g < 32; ++g) qf[g] = 0.f;
  }
  dma(0, 0);
  if (NS == 3 && a.nkv > 1) {
    dma(1, 1);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // tile 0 (and Q) landed, tile 1 in flight
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // two stages: tile 1 is iteration 0's to issue, whatever nkv is
  }
  __builtin_amdgcn_s_barrier();

  x3_f16 oacc[2];
#pragma unroll
  for (int dm = 0; dm < 2; ++dm)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dm][r] = 0.f;
  float m_run = -INFINITY, l_half = 0.f;
  // One tile.  stage: the ring stage it reads; NM = 2: the whole tile, NM = 1: a last tile with at most 32 live rows -- its second M tile is all past T and is
  // left out of both products (k_attn_f32's header says what that changes).
  auto tile = [&](int it, int stage, auto nm) __attribute__((always_inline)) {
    constexpr int NM = decltype(nm)::value;
    const bool ahead = it + (NS - 1) < a.nkv;
    // the stage tile it - 1 left: every wave's reads of it returned before the barrier that ended iteration it - 1
    if (ahead) dma(it + (NS - 1), (stage + NS - 1) % NS);
    const uint8_t* sv = at_lds + stage * AF_STAGE + AF_TILE;
    if (live) {
      // ---- S^T = K Q^T (pre-scaled logits)
      x3_f16 s[2];
      af_st<NM>(kp, stage, qf, s);
      if ((it + 1) * AT_BK > a.T) {   // last tile: rows past T (a uniform branch off the hot path)
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (it * AT_BK + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * kh >= a.T) s[m][r] = -INFINITY;
      }
      // ---- online softmax: running maximum over both lane halves, rescale only when it grew somewhere in the wave
      float mx = s[0][0];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[m][r]);
      {   // the other lane half's maximum by v_permlane32_swap (both results hold one half's values in all 64 lanes), not through the LDS pipe
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      const float m_new = fmaxf(m_run, mx);
      if (__any(m_new > m_run)) {
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // 0 on the first tile (m_run = -inf), exactly 1 where the maximum did not grow
#pragma unroll
        for (int dm = 0; dm < 2; ++dm)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[dm][r] *= alpha;
        l_half *= alpha;
        m_run = m_new;
      }
      float ps = 0.f;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[m][r] = __builtin_amdgcn_exp2f(s[m][r] - m_run); ps += s[m][r]; }
      l_half += ps;
      // ---- O^T += V^T P^T
      af_pv<0>(sv, s, va, oacc);
      if (NM == 2) af_pv<1>(sv, s, va, oacc);
    }
    // before the barrier: this wave's reads of this stage have returned (behind it, the next iteration's DMA overwrites that stage: tile it + 3 / it + 2) and
    // tile it + 1 has landed (three stages: the four DMA instructions of tile it + 2 may stay in flight; two stages: tile it + 1 is the only one in flight)
    if (NS == 3 && ahead) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  // The tile loop is unrolled over the ring: copy u of the body serves the tiles it = u (mod NS), so the stage it reads (u) and the stage its DMA fills are
  // compile-time constants and every LDS address of the loop is a loop-invariant register plus an immediate.  Waits and barrier are per tile as before -- each
  // copy ends with the counted wait and the one barrier of its tile -- and the loop may end behind any copy.  A last tile with at most 32 live rows (T mod 64
  // in 1 .. 32) is taken out of the loop: one more copy of the body, NM = 1, its stage a run-time value.
  const int nfull = (a.nkv - 1) * AT_BK + 32 >= a.T ? a.nkv - 1 : a.nkv;
  for (int it0 = 0; it0 < nfull; it0 += NS) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      if (it0 + u >= nfull) break;
      tile(it0 + u, u, af_ic<2>());
    }
  }
  if (nfull < a.nkv) tile(nfull, nfull % NS, af_ic<1>());

  // ---- epilogue: out[b][q][h][16 g + 8 kh + 2 j + dm] = O^T_dm[register 4 g + j] / l
  const float l_tot = l_half + __shfl_xor(l_half, 32, 64);
  const int q = q0 + li;
  if (q < a.T) {
    float* op = out + (((size_t)b * a.T + q) * a.H + h) * AT_D + 8 * kh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 lo = {oacc[0][4 * g] / l_tot, oacc[1][4 * g] / l_tot, oacc[0][4 * g + 1] / l_tot, oacc[1][4 * g + 1] / l_tot};
      const float4 hi = {oacc[0][4 * g + 2] / l_tot, oacc[1][4 * g + 2] / l_tot, oacc[0][4 * g + 3] / l_tot, oacc[1][4 * g + 3] / l_tot};
      *reinterpret_cast<float4*>(op + 16 * g) = lo;
      *reinterpret_cast<float4*>(op + 16 * g + 4) = hi;
    }
  }
}

template <int NW, int NS>
static bool af_launch(hipStream_t s, const float* qkv, float* out, vd_at_args a) {
  static bool attr_set[64] = {};
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_attn_f32<NW, NS>), AF_LDS(NS)}}, attr_set)) return false;   // per device (vd3d_kernels.h)
  a.nqb = (a.T + NW * 32 - 1) / (NW * 32);
  const int groups = (a.B * a.H + 7) / 8;
  hipLaunchKernelGGL((k_attn_f32<NW, NS>), dim3((unsigned)(8 * groups * a.nqb)), dim3(NW * 64), AF_LDS(NS), s, qkv, out, a);
  return true;
}

// form: 8 / 4 = the workgroup's wave count, 0 = the library's choice.
// Form 0, from profiles/r15_attn_f32_forms.md (MI355X, 256 CUs): the 4-wave form where the 8-wave grid is at least four rounds of the chip (1 024 workgroups),
// the 8-wave form below that.  Grounds: alone, the 4-wave form is faster wherever the 8-wave grid ends in a short round (16 x 2 443 x 12: 7.5 rounds, 2.55 ->
// 2.44 ms; 16 x 1 370 x 6: 2.25 rounds, 0.552 -> 0.470 ms) and level where it does not (16 x 2 443 x 16: 10 rounds); no shape was found where it is slower alone.
// Inside the depth + DIBR step the long grid keeps most of that (4K DA-V2-Base: 113.31 -> 112.30 ms per step, 4.4 x the spread), the short one does not: at
// 1080p DA-V2-Small the attention shares the chip with the pixel kernels of the other streams for its whole length (1.33 ms per call in the step against 0.55
// alone) and the step came out 0.4 % SLOWER with the 4-wave form (381.0 -> 379.5 pairs/s, three alternating runs each, 1.9 x the spread).  Nothing was measured
// between 576 and 1 920 workgroups: the threshold is the round number in between, not a measured crossover.
bool vd_launch_attn_f32(hipStream_t s, const float* qkv, int B, int T, int H, int D, float scale, float* out, int form) {
  if (B < 1 || T < 1 || H < 1 || D != AT_D || (long long)B * H > 65535) return false;
  if (form != 0 && form != 4 && form != 8) return false;
  if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return false;
  vd_at_args a;
  a.B = B; a.H = H; a.T = T;
  a.nq32 = (T + 31) / 32; a.nkv = (T + AT_BK - 1) / AT_BK; a.nqb = 0;
  a.c = scale * 1.44269504088896340736f;
  if (form == 0) form = 8LL * ((B * H + 7) / 8) * ((T + AT_BQ - 1) / AT_BQ) >= 1024 ? 4 : 8;
  return form == 4 ? af_launch<4, 2>(s, qkv, out, a) : af_launch<8, 3>(s, qkv, out, a);
}

static bool at_mode_ok(int mode) { return mode == 0 || mode == 1; }
long long vd_attn_x3_workspace_bytes(int B, int T, int H, int D, int mode) {
  if (B < 1 || T < 1 || H < 1 || D != AT_D || !at_mode_ok(mode)) return -1;
  const long long nq32 = (T + 31) / 32, nkv = (T + AT_BK - 1) / AT_BK;
  const long long qblk = mode == 0 ? AT_QBLK(0) : AT_QBLK(1), tile = mode == 0 ? AT_TILE(0) : AT_TILE(1);
  return (long long)B * H * (nq32 * qblk * 16 + 2 * nkv * tile);
}

template <int MODE>
static bool at_launch(hipStream_t s, const float* qkv, int B, int T, int H, float scale, void* ws, float* out) {
  static bool attr_set[64] = {};
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_attn_bf16x3<MODE>), AT_LDS(MODE)}}, attr_set)) return false;
  vd_at_args a;
  a.B = B; a.H = H; a.T = T;
  a.nq32 = (T + 31) / 32; a.nkv = (T + AT_BK - 1) / AT_BK; a.nqb = (T + AT_BQ - 1) / AT_BQ;
  a.c = scale * 1.44269504088896340736f;
  if (MODE == 1) a.c *= 1.0f / (AT_QKV_SCALE * AT_QKV_SCALE);   // the logits were computed from 2^4 q and 2^4 k (exact rescale)
  uint4* Qimg = reinterpret_cast<uint4*>(ws);
  uint4* Kimg = Qimg + (size_t)B * H * a.nq32 * AT_QBLK(MODE);
  uint4* Vimg = Kimg + (size_t)B * H * a.nkv * (AT_TILE(MODE) / 16);
  const int rows_max = a.nkv * 64 > a.nq32 * 32 ? a.nkv * 64 : a.nq32 * 32;   // Q / K: rows * 8 threads; V^T: tiles * 512 threads = the same count
  hipLaunchKernelGGL(k_attn_x3_prep<MODE>, dim3((unsigned)((rows_max * 8 + 255) / 256), (unsigned)(B * H), 3), dim3(256), 0, s, qkv, a, Qimg, Kimg, Vimg);
  const int groups = (B * H + 7) / 8;
  hipLaunchKernelGGL(k_attn_bf16x3<MODE>, dim3((unsigned)(8 * groups * a.nqb)), dim3(AT_NT), AT_LDS(MODE), s, Qimg, Kimg, Vimg, out, a);
  return true;
}

bool vd_launch_attn_x3(hipStream_t s, const float* qkv, int B, int T, int H, int D, float scale, void* ws, float* out, int mode) {
  if (vd_attn_x3_workspace_bytes(B, T, H, D, mode) < 0) return false;
  if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(ws) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return false;
  if ((long long)B * H > 65535) return false;
  return mode == 0 ? at_launch<0>(s, qkv, B, T, H, scale, ws, out) : at_launch<1>(s, qkv, B, T, H, scale, ws, out);
}
