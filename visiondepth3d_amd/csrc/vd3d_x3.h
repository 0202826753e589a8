// vd3d_x3.h -- the split arithmetic every matrix-core kernel of this library shares (vd3d_gemm.hip, vd3d_attn.hip, vd3d_conv2.hip, vd3d_conv_x3.hip): the
// vector and address-space types, the exact three-term bf16 split, the two-term fp16 split and the MFMA that consumes their fragments.  Device code only; every
// function is forced inline and compiles to exactly the instructions written here.
//
// bf16x3 (MODE 0).  A float32 number is EXACTLY the sum of three bf16 numbers (8 significant bits each, 3 x 8 = 24: truncate, subtract, truncate, subtract --
// the last remainder has <= 8 bits).  bf16 has float32's exponent: no pre-scaling, no range limit; NaN / Inf in give NaN out.  Of the nine products of
// (x1 + x2 + x3)(w1 + w2 + w3), each exact in float32, the kernels keep six and drop x2 w3 + x3 w2 + x3 w3 <= 2^-23 |x w| (the size of one float32 rounding).
// fp16x2 (MODE 1).  a ~ h1 + h2 with h1 = fp16(a), h2 = fp16(a - h1), both round-to-nearest: 22 significant bits, |a - h1 - h2| <= 2^-22 |a| while h2 stays a
// normal fp16 number (|a| >= 2^-2 for unscaled data; below that the absolute error is <= 2^-25).  |a| must stay below 65 504: the callers scale by exact powers of
// two where their data needs it (weight rows in the GEMM, vd3d_conv2.hip and vd3d_conv_x2t.hip, q / k / v and the probabilities in the attention).
#pragma once
#include "vd3d_dev.h"

// 8 bf16 or 8 fp16 = one MFMA A / B fragment (4 VGPRs), carried as shorts.  LDS that LDS-DMA fills is read as THIS type and bit-cast: hipcc orders a float4 LDS
// read behind every LDS-DMA in flight (s_waitcnt vmcnt(0)), not a short-vector read.
typedef short x3_s8 __attribute__((ext_vector_type(8)));
typedef __bf16 x3_b8 __attribute__((ext_vector_type(8)));
typedef _Float16 x3_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 x3_h4 __attribute__((ext_vector_type(4)));
typedef float x3_f16 __attribute__((ext_vector_type(16)));      // one 32 x 32 accumulator tile per wave
typedef uint32_t x3_u2 __attribute__((ext_vector_type(2)));
typedef uint32_t x3_u4 __attribute__((ext_vector_type(4)));
// the operands of __builtin_amdgcn_global_load_lds (LDS-DMA: global -> LDS without registers)
typedef __attribute__((address_space(3))) void* x3_lds_vp;
typedef const __attribute__((address_space(1))) void* x3_glb_vp;

// exact split by truncation: a == t1 + t2 + t3, the terms as float32 words whose low 16 bits are zero
VD_DEV void x3_split(float a, uint32_t& t1, uint32_t& t2, uint32_t& t3) {
  t1 = __float_as_uint(a) & 0xffff0000u;
  const float r1 = a - __uint_as_float(t1);
  t2 = __float_as_uint(r1) & 0xffff0000u;
  const float r2 = r1 - __uint_as_float(t2);
  t3 = __float_as_uint(r2);   // <= 8 significant bits: its low half is zero
}
// the high halves of two words as one: lo >> 16 | hi & 0xffff0000 (two bf16)
VD_DEV uint32_t x3_pack(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }
// eight float32 (the k = 8 kh .. 8 kh + 7 of one row) -> the three bf16 fragments of that lane
VD_DEV void x3_split8(const float v[8], x3_s8 out[3]) {
  uint32_t t1[8], t2[8], t3[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x3_split(v[e], t1[e], t2[e], t3[e]);
  const x3_u4 p1 = {x3_pack(t1[0], t1[1]), x3_pack(t1[2], t1[3]), x3_pack(t1[4], t1[5]), x3_pack(t1[6], t1[7])};
  const x3_u4 p2 = {x3_pack(t2[0], t2[1]), x3_pack(t2[2], t2[3]), x3_pack(t2[4], t2[5]), x3_pack(t2[6], t2[7])};
  const x3_u4 p3 = {x3_pack(t3[0], t3[1]), x3_pack(t3[2], t3[3]), x3_pack(t3[4], t3[5]), x3_pack(t3[6], t3[7])};
  out[0] = __builtin_bit_cast(x3_s8, p1); out[1] = __builtin_bit_cast(x3_s8, p2); out[2] = __builtin_bit_cast(x3_s8, p3);
}

// the two fp16 terms of four or eight float32; the form with `pre` splits v[e] * pre (a power of two: exact), the form without it multiplies nothing
VD_DEV void x3_split4_h(const float v[4], x3_h4& h1, x3_h4& h2) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { const _Float16 t = (_Float16)v[e]; h1[e] = t; h2[e] = (_Float16)(v[e] - (float)t); }
}
VD_DEV void x3_split8_h(const float v[8], x3_s8 out[2]) {
  x3_h8 h1, h2;
#pragma unroll
  for (int e = 0; e < 8; ++e) { const _Float16 t = (_Float16)v[e]; h1[e] = t; h2[e] = (_Float16)(v[e] - (float)t); }
  out[0] = __builtin_bit_cast(x3_s8, h1); out[1] = __builtin_bit_cast(x3_s8, h2);
}
VD_DEV void x3_split8_h(const float v[8], float pre, x3_s8 out[2]) {
  x3_h8 h1, h2;
#pragma unroll
  for (int e = 0; e < 8; ++e) { const float x = v[e] * pre; const _Float16 t = (_Float16)x; h1[e] = t; h2[e] = (_Float16)(x - (float)t); }
  out[0] = __builtin_bit_cast(x3_s8, h1); out[1] = __builtin_bit_cast(x3_s8, h2);
}
template <int MODE> VD_DEV void x3_split8_m(const float v[8], x3_s8* out) {
  if (MODE == 0) x3_split8(v, out); else x3_split8_h(v, out);
}
template <int MODE> VD_DEV void x3_split8_m(const float v[8], float pre, x3_s8* out) {   // bf16x3 needs no pre-scale and takes none
  if (MODE == 0) x3_split8(v, out); else x3_split8_h(v, pre, out);
}

// D = A B + C on one 32 x 32 x 16 tile, float32 accumulation: bf16 fragments (MODE 0) or fp16 fragments (MODE 1)
template <int MODE> VD_DEV x3_f16 x3_mfma(const x3_s8& a, const x3_s8& b, const x3_f16& c) {
  if (MODE == 0) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x3_b8, a), __builtin_bit_cast(x3_b8, b), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(x3_h8, a), __builtin_bit_cast(x3_h8, b), c, 0, 0, 0);
}
