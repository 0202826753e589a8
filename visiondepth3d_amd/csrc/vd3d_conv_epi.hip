// vd3d_conv_epi.hip -- vd3d_conv3x3_epi: the stride-1 tile convolution of vd3d_conv_x3.h with the glue of a pre-activation residual unit in its epilogue
// (cx_conv's EPI 2), in both arithmetics: MODE 0 (bf16x3) reads the weight image of vd3d_conv3x3_x3_pack_weights, MODE 1 (fp16x2) the one of
// vd3d_conv3x3_s1_x2_pack_weights -- no image format of its own.  The sum is formed exactly as the bias-free kernel of the mode forms it (same tile, same
// K order, same two accumulators, acc + lo, times colscale in MODE 1), over X or -- relu_in -- over relu(X) with the ReLU applied to the staged pixels in
// front of the split; then vd3d_nhwc_bias_act_f32's chain runs on the value in registers:
//   v = u; [v = v + bias[oc]]; [v = v + r1[p][oc]]; [v = r2[p][oc] + v]; [v = max(v, 0)]; Y = v; [Yrelu = max(v, 0)]
// The library is built with -ffp-contract=off, so Y and Yrelu EQUAL what [relu ->] bias-free convolution -> vd3d_nhwc_bias_act_f32 writes, and the maps that
// pair moves through memory between its launches (the bare sum, twice; the ReLU'd input) are never written.
// C_out 32 / 64 / 128 / 256 on the instantiations of the bare kernels (8 x 1 waves; 4 x 2 with one or two N tiles; 256 as two slices on the grid's z axis).
// The output tile of a workgroup is read by no other workgroup only if Y / Yrelu are not X: the launcher refuses any overlap of an output with an input.
#include "vd3d_dev.h"
#include "vd3d_conv_x3.h"

static_assert(cx_lds_m(0, 128) == 155392 && cx_lds_m(1, 128) == 100864, "the LDS plans of the bare kernels");

static bool ce_overlap(const void* p, long long pn, const void* q, long long qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return p && q && a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

template <int MODE>
static bool ce_launch(hipStream_t s, dim3 grid, int Cout, const vd_cx_args& a) {
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_conv_epi<MODE, 8, 1>), cx_lds_m(MODE, 32)}, {reinterpret_cast<const void*>(k_conv_epi<MODE, 4, 1>), cx_lds_m(MODE, 64)},
                     {reinterpret_cast<const void*>(k_conv_epi<MODE, 4, 2>), cx_lds_m(MODE, 128)}}, attr_set)) return false;
  if (Cout == 32) hipLaunchKernelGGL((k_conv_epi<MODE, 8, 1>), grid, dim3(CX_NT), cx_lds_m(MODE, 32), s, a);
  else if (Cout == 64) hipLaunchKernelGGL((k_conv_epi<MODE, 4, 1>), grid, dim3(CX_NT), cx_lds_m(MODE, 64), s, a);
  else hipLaunchKernelGGL((k_conv_epi<MODE, 4, 2>), grid, dim3(CX_NT), cx_lds_m(MODE, 128), s, a);   // 128, or 256 as two slices
  return true;
}

// 0: launched; 1: shape not built; 2: pointer rule (alignment, batch, map); 3: an output overlaps an input or the other output; 4: LDS opt-in failed
int vd_launch_conv3x3_epi(hipStream_t s, int mode, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, int flags, const float* bias,
                          const float* r1, const float* r2, float* Y, float* Yrelu) {
  const long long wb = mode == 0 ? vd_conv3x3_x3_weight_bytes(Cin, Cout) : vd_conv3x3_s1_x2_weight_bytes(Cin, Cout);
  if (wb < 0) return 1;
  const uint8_t* wi = reinterpret_cast<const uint8_t*>(wimg);
  const float* cs = mode == 0 ? nullptr : reinterpret_cast<const float*>(wi + wb - 64 - (long long)Cout * 4);   // MODE 1: colscale[C_out] in front of the zero page
  vd_cx_args a;
  dim3 grid;
  if (!cx_dense_args(CX_K3S1, X, B, H, W, Cin, wimg, Cout, Y, cs, reinterpret_cast<const float*>(wi + wb - 64), a, grid)) return 2;
  for (const void* p : {(const void*)bias, (const void*)r1, (const void*)r2, (const void*)Yrelu})
    if (reinterpret_cast<uintptr_t>(p) & 3) return 2;
  const long long npix = (long long)B * H * W, xn = npix * Cin * 4, yn = npix * Cout * 4;
  for (const float* o : {(const float*)Y, (const float*)Yrelu})
    if (ce_overlap(o, yn, X, xn) || ce_overlap(o, yn, r1, yn) || ce_overlap(o, yn, r2, yn) || ce_overlap(o, yn, bias, (long long)Cout * 4) || ce_overlap(o, yn, wimg, wb))
      return 3;
  if (ce_overlap(Y, yn, Yrelu, yn)) return 3;
  a.bias = bias; a.R = r1; a.R2 = r2; a.Y2 = Yrelu; a.r_stride = Cout;
  a.relu_in = flags & 1; a.relu = (flags >> 1) & 1;
  return (mode == 0 ? ce_launch<0>(s, grid, Cout, a) : ce_launch<1>(s, grid, Cout, a)) ? 0 : 4;
}
