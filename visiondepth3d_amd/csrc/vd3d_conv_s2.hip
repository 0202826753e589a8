// vd3d_conv_s2.hip -- vd3d_conv3x3_s2_x3: the 3 x 3 / stride 2 / padding 1 convolution of the DPT reassemble stage (384 / 768 / 1024 -> same) in the bf16x3
// arithmetic, on the tile-convolution kernel of vd3d_conv_x3.h in its K3S2 geometry (the space-to-depth view without zero-weight taps: vd3d_conv_x3.hip's
// header comment) with the workgroup shape of the DPT stride-1 convolution: 128 output channels per workgroup (4 x 2 waves, two tile rows and two N tiles per
// wave), C_out = 128 n as n channel slices on the grid's z axis, the bare `acc + lo` epilogue.  Float32 NHWC in and out, dense maps (pitches C_in and C_out),
// output (H+1)/2 x (W+1)/2.  Every slice stages and splits the input tile again (four stagings per 16 channels); at the reassemble stage's map sizes the
// workgroups are few and the launch is latency-bound either way.
// The launch here is the kernel and its LDS opt-in; the checks, the argument block and the grid are cx_dense_args's (vd3d_conv_x3.h).
// The weight image is packed by vd3d_conv_x3.hip (k_conv_x3_pack, kind K3S2: [slice][step 9 nchunk][term 3][k-half 2][oc 128][8 bf16] + the zero page).
#include "vd3d_conv_x3.h"

static_assert(cx_lds(128) <= 163840, "LDS plan");

bool vd_launch_conv3x3_s2_x3(hipStream_t s, const float* X, int B, int H, int W, int Cin, const void* wimg, int Cout, float* Y) {
  const long long wb = vd_conv3x3_s2_x3_weight_bytes(Cin, Cout);
  vd_cx_args a;
  dim3 grid;
  if (wb < 0 || !cx_dense_args(CX_K3S2, X, B, H, W, Cin, wimg, Cout, Y, nullptr, reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(wimg) + wb - 64), a, grid))
    return false;
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_conv_x3<CX_K3S2, 4, 2, false>), cx_lds(128)}}, attr_set)) return false;
  hipLaunchKernelGGL((k_conv_x3<CX_K3S2, 4, 2, false>), grid, dim3(CX_NT), cx_lds(128), s, a);
  return true;
}
