// vd3d_head_upconv.hip -- the fine half of the float32 head's first convolution in "coarse GEMM + fine gather" form.
//
// The last fusion layer's 1 x 1 projection P (bias b_p), the align_corners bilinear up-sampling U and the head's bias-free 3 x 3 convolution (taps W_t, zero
// padding) have nothing non-linear between them; U acts per channel and W_t per pixel, so with S_t the shift of tap t on the FINE grid (zero outside it)
//     conv1(U(P h + b_p)) = sum over the 9 taps t of  S_t U ( (W_t P) h + W_t b_p )
// All channel mixing is one GEMM on the coarse map (depth.py head_upconv_compose: 128 -> 9 x 64 channels, a quarter of the fine map's pixels); this file is what
// remains on the fine map:
//     y1[b][Y][X][o] = sum over t = 3 ky + kx = 0 .. 8 ascending with (Y + ky - 1, X + kx - 1) inside [0, H) x [0, W)
//                      of  bilinear(Z[b][:][:][t][o]; Y + ky - 1, X + kx - 1)
// Z float32 [B][h][w][9][CO] -> y1 float32 NHWC [B][H][W][CO] (conv1 WITHOUT its bias).  The bilinear sample takes upsample_bilinear_f32_body's coordinates
// operation for operation (vd3d_netops.hip): s = (float)(h - 1) / (float)(H - 1), f = s * (float)y, i0 = (int)f, i1 = i0 + (i0 < h - 1), l1 = f - (float)i0,
// l0 = 1.f - l1.  Association (NOT the up-sampler's): per tap the four corner weights ly_a * lx_b are rounded products, and every output value is ONE chain
//     acc = 0;  acc = fmaf(w, z, acc)   taps ascending, corners (y0, x0), (y0, x1), (y1, x0), (y1, x1)
// of at most 36 fused multiply-adds, summed by one lane: no atomics, no split; bits depend neither on the batch nor on the call.
//
// Work split: a workgroup = one fine tile of at most HU_TH x HU_TW pixels x one chunk of HU_CC = 8 output channels.  The coarse pixels its 3 x 3 windows reach
// (the tile + 1 fine pixel around it: at most HU_CY x HU_CX coarse pixels) are staged in LDS for all 9 taps as [cy][cx][tap][8] (69 120 bytes: two workgroups per
// CU); at the factor-2 shapes of the depth head a 16 x 32 tile reaches 10 x 18 coarse pixels, a halo re-read of 1.41 x.  The host shrinks the tile (whole-map exact
// search with the kernel's own float operations) until every tile's reach fits, so any H x W is served up to a down-sampling factor of about HU_CY - 3.  Row and
// column taps (corner offsets and weights) are uniform along a tile's rows and columns: two small LDS tables.  A thread = 4 channels (16 bytes) of one pixel:
// 36 ds_read_b128 and 144 FMAs; loads and stores are 16 bytes per lane, 32 contiguous bytes per (pixel, tap).  The channel chunks of one tile read the same
// 128-byte lines of Z: the workgroup index is remapped so that they follow each other on ONE XCD (workgroups are dealt round-robin to the 8 XCDs) and meet in its L2.
#include "vd3d_dev.h"
#include "vd3d_kernels.h"

#define HU_TH 16
#define HU_TW 32
#define HU_CY 12
#define HU_CX 20
#define HU_CC 8
#define HU_NT 256
#define HU_XCD 8
#define HU_LD ((HU_CY * HU_CX * 18 + HU_NT - 1) / HU_NT)   // 16-byte loads per lane that stage a full window (17)
constexpr int hu_lds() { return HU_CY * HU_CX * 9 * HU_CC * 4; }
static_assert(2 * (hu_lds() + (HU_TH + 2 + HU_TW + 2) * 16) <= 160 * 1024, "two workgroups per CU");

struct vd_hu_args {
  int h, w, H, W;        // coarse / fine map
  int th, tw;            // the tile (<= HU_TH x HU_TW) the host fitted
  int nty, ntx, ntiles;  // tiles per frame column / row, B * nty * ntx
  float sh, sw;
};

// one output quad: the chain over the 9 taps x 4 corners in the stated order; CHECK: skip the taps outside the map (offset -1 in the tables)
template <bool CHECK>
VD_DEV float4 hu_taps(const float4* zs, const int* r_o0, const int* r_o1, const float* r_l0, const float* r_l1, const int* c_o0, const int* c_o1, const float* c_l0,
                      const float* c_l1, int ty, int tx, int half) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int ro0 = r_o0[ty + ky], ro1 = r_o1[ty + ky];
    if (CHECK && ro0 < 0) continue;
    const float ly0 = r_l0[ty + ky], ly1 = r_l1[ty + ky];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int co0 = c_o0[tx + kx], co1 = c_o1[tx + kx];
      if (CHECK && co0 < 0) continue;
      const float lx0 = c_l0[tx + kx], lx1 = c_l1[tx + kx];
      const float w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1;
      const int t2 = (3 * ky + kx) * 2 + half;
      const float4 z00 = zs[(ro0 + co0) * 18 + t2], z01 = zs[(ro0 + co1) * 18 + t2];
      const float4 z10 = zs[(ro1 + co0) * 18 + t2], z11 = zs[(ro1 + co1) * 18 + t2];
      acc.x = __builtin_fmaf(w00, z00.x, acc.x); acc.y = __builtin_fmaf(w00, z00.y, acc.y); acc.z = __builtin_fmaf(w00, z00.z, acc.z); acc.w = __builtin_fmaf(w00, z00.w, acc.w);
      acc.x = __builtin_fmaf(w01, z01.x, acc.x); acc.y = __builtin_fmaf(w01, z01.y, acc.y); acc.z = __builtin_fmaf(w01, z01.z, acc.z); acc.w = __builtin_fmaf(w01, z01.w, acc.w);
      acc.x = __builtin_fmaf(w10, z10.x, acc.x); acc.y = __builtin_fmaf(w10, z10.y, acc.y); acc.z = __builtin_fmaf(w10, z10.z, acc.z); acc.w = __builtin_fmaf(w10, z10.w, acc.w);
      acc.x = __builtin_fmaf(w11, z11.x, acc.x); acc.y = __builtin_fmaf(w11, z11.y, acc.y); acc.z = __builtin_fmaf(w11, z11.z, acc.z); acc.w = __builtin_fmaf(w11, z11.w, acc.w);
    }
  }
  return acc;
}

template <int CO>
__global__ __launch_bounds__(HU_NT) void k_head_upconv_gather_f32(const float4* __restrict__ z, float4* __restrict__ out, vd_hu_args a) {
  constexpr int NCH = CO / HU_CC, C4 = CO / 4;
  extern __shared__ float4 hu_zs[];
  __shared__ int r_o0[HU_TH + 2], r_o1[HU_TH + 2], c_o0[HU_TW + 2], c_o1[HU_TW + 2];      // corner offsets in coarse pixels of the staged window; -1: outside the map
  __shared__ float r_l0[HU_TH + 2], r_l1[HU_TH + 2], c_l0[HU_TW + 2], c_l1[HU_TW + 2];
  const int tid = threadIdx.x;
  const int k = blockIdx.x / HU_XCD;
  const int chunk = k % NCH, tile = (k / NCH) * HU_XCD + (int)(blockIdx.x % HU_XCD);
  if (tile >= a.ntiles) return;
  const int txi = tile % a.ntx, tr = tile / a.ntx, tyi = tr % a.nty, b = tr / a.nty;
  const int Y0 = tyi * a.th, X0 = txi * a.tw;
  // the coarse window: corners of the first and the last fine row / column the tile's windows reach (the coordinate is monotonic in y)
  const int ya = Y0 > 0 ? Y0 - 1 : 0, yb = Y0 + a.th < a.H ? Y0 + a.th : a.H - 1;
  const int xa = X0 > 0 ? X0 - 1 : 0, xb = X0 + a.tw < a.W ? X0 + a.tw : a.W - 1;
  const int cy_lo = (int)(a.sh * (float)ya), cyb = (int)(a.sh * (float)yb), cy_hi = cyb + (cyb < a.h - 1 ? 1 : 0);
  const int cx_lo = (int)(a.sw * (float)xa), cxb = (int)(a.sw * (float)xb), cx_hi = cxb + (cxb < a.w - 1 ? 1 : 0);
  const int ncy = cy_hi - cy_lo + 1, ncx = cx_hi - cx_lo + 1;
  if (ncy > HU_CY || ncx > HU_CX) return;   // the host fitted the tile: never taken

  if (tid < a.th + 2) {
    const int y = Y0 - 1 + tid;
    int o0 = -1, o1 = -1;
    float l0 = 0.f, l1 = 0.f;
    if (y >= 0 && y < a.H) {
      const float fy = a.sh * (float)y;
      const int y0 = (int)fy;
      const int y1 = y0 + (y0 < a.h - 1 ? 1 : 0);
      l1 = fy - (float)y0; l0 = 1.f - l1;
      o0 = (y0 - cy_lo) * ncx; o1 = (y1 - cy_lo) * ncx;
    }
    r_o0[tid] = o0; r_o1[tid] = o1; r_l0[tid] = l0; r_l1[tid] = l1;
  }
  if (tid >= 64 && tid < 64 + a.tw + 2) {
    const int c = tid - 64, x = X0 - 1 + c;
    int o0 = -1, o1 = -1;
    float l0 = 0.f, l1 = 0.f;
    if (x >= 0 && x < a.W) {
      const float fx = a.sw * (float)x;
      const int x0 = (int)fx;
      const int x1 = x0 + (x0 < a.w - 1 ? 1 : 0);
      l1 = fx - (float)x0; l0 = 1.f - l1;
      o0 = x0 - cx_lo; o1 = x1 - cx_lo;
    }
    c_o0[c] = o0; c_o1[c] = o1; c_l0[c] = l0; c_l1[c] = l1;
  }

  // stage Z[b][cy_lo .. cy_hi][cx_lo .. cx_hi][0 .. 8][8 chunk .. 8 chunk + 7]: LDS quad i = ((cyl ncx + cxl) 9 + tap) 2 + half
  {
    const int rowq = ncx * 18, n4 = ncy * rowq;
    const float4* zb = z + ((size_t)b * a.h + cy_lo) * a.w * (9 * C4) + (size_t)cx_lo * (9 * C4) + chunk * 2;
    const int zrow = a.w * (9 * C4);   // quads per coarse row (the host keeps it below 2^31)
    // the whole window in ONE batch of loads per lane (the latency is paid once).  No branch: a lane past the end loads AND stores the last quad again (the same
    // value to the same place), so that the compiler keeps the loads together instead of sinking each into its store's branch
    float4 v[HU_LD];
    int li[HU_LD];
    const int stepq = HU_NT / rowq, stepr = HU_NT - stepq * rowq;   // uniform: quad i + HU_NT is stepq rows and stepr quads on (one more row on a carry)
    int cyl = tid / rowq, j = tid - cyl * rowq;
#pragma unroll
    for (int u = 0; u < HU_LD; ++u) {
      const bool in = tid + u * HU_NT < n4;
      const int cy_u = in ? cyl : ncy - 1, j_u = in ? j : rowq - 1;
      const int cxl = j_u / 18, rr = j_u - cxl * 18;
      li[u] = in ? tid + u * HU_NT : n4 - 1;
      v[u] = (zb + (size_t)cy_u * zrow)[cxl * (9 * C4) + (rr >> 1) * C4 + (rr & 1)];
      cyl += stepq; j += stepr;
      if (j >= rowq) { j -= rowq; ++cyl; }
    }
    __builtin_amdgcn_sched_barrier(0);   // keeps the address arithmetic ahead of the loads: they issue back to back, the stores drain them with up to ten in flight
#pragma unroll
    for (int u = 0; u < HU_LD; ++u) hu_zs[li[u]] = v[u];
  }
  __syncthreads();

  const int items = a.th * a.tw * 2;
  for (int it = tid; it < items; it += HU_NT) {
    const int half = it & 1, px = it >> 1;
    const int ty = px / a.tw, tx = px - ty * a.tw;
    const int Y = Y0 + ty, X = X0 + tx;
    if (Y >= a.H || X >= a.W) continue;
    // a pixel whose 9 taps all lie inside the map (all but the map's border) takes the path without a branch, where the 36 LDS reads can be issued ahead of the chain
    const bool inner = r_o0[ty] >= 0 && r_o0[ty + 2] >= 0 && c_o0[tx] >= 0 && c_o0[tx + 2] >= 0;
    const float4 acc = inner ? hu_taps<false>(hu_zs, r_o0, r_o1, r_l0, r_l1, c_o0, c_o1, c_l0, c_l1, ty, tx, half)
                             : hu_taps<true>(hu_zs, r_o0, r_o1, r_l0, r_l1, c_o0, c_o1, c_l0, c_l1, ty, tx, half);
    (out + ((size_t)b * a.H + Y) * a.W * C4)[X * C4 + chunk * 2 + half] = acc;
  }
}

// the largest tile edge t <= tmax whose every tile along one axis reaches at most cap coarse pixels (the kernel's own float operations); 0: none
static int hu_fit(int n, int nc, float s, int tmax, int cap) {
  for (int t = tmax; t >= 1; --t) {
    bool ok = true;
    for (long long p0 = 0; p0 < n && ok; p0 += t) {
      const int pa = p0 > 0 ? (int)p0 - 1 : 0, pb = p0 + t < n ? (int)(p0 + t) : n - 1;
      const int lo = (int)(s * (float)pa), hb = (int)(s * (float)pb), hi = hb + (hb < nc - 1 ? 1 : 0);
      if (lo < 0 || hi > nc - 1 || hi - lo + 1 > cap) ok = false;
    }
    if (ok) return t;
  }
  return 0;
}

static bool hu_plan(int B, int h, int w, int H, int W, int Cout, vd_hu_args& a) {
  if ((Cout != 64 && Cout != 32) || B < 1 || h < 1 || w < 1 || H < 2 || W < 2) return false;
  if ((long long)w * 9 * Cout >= (1ll << 31) || (long long)W * Cout >= (1ll << 31)) return false;   // 32-bit offsets inside a row; rows and frames are 64-bit
  a.h = h; a.w = w; a.H = H; a.W = W;
  a.sh = (float)(h - 1) / (float)(H - 1); a.sw = (float)(w - 1) / (float)(W - 1);                   // area_pixel_compute_scale, align_corners
  a.th = hu_fit(H, h, a.sh, HU_TH, HU_CY); a.tw = hu_fit(W, w, a.sw, HU_TW, HU_CX);
  if (a.th < 1 || a.tw < 1) return false;                                                          // a down-sampling factor no tile serves
  a.nty = (H + a.th - 1) / a.th; a.ntx = (W + a.tw - 1) / a.tw;
  const long long nt = (long long)B * a.nty * a.ntx;
  if (((nt + HU_XCD - 1) / HU_XCD) * HU_XCD * (Cout / HU_CC) >= (1ll << 31)) return false;           // the grid
  a.ntiles = (int)nt;
  return true;
}

bool vd_head_upconv_shape_ok(int B, int h, int w, int H, int W, int Cout) {
  vd_hu_args a;
  return hu_plan(B, h, w, H, W, Cout, a);
}

bool vd_launch_head_upconv_gather_f32(hipStream_t s, const float* z, int B, int h, int w, int H, int W, int Cout, float* out) {
  vd_hu_args a;
  if (!hu_plan(B, h, w, H, W, Cout, a)) return false;
  static bool attr_set[64] = {};   // per device: the > 64 KB dynamic-LDS opt-in is a per-device function attribute (vd3d_kernels.h)
  if (!vd_lds_optin({{reinterpret_cast<const void*>(k_head_upconv_gather_f32<64>), hu_lds()}, {reinterpret_cast<const void*>(k_head_upconv_gather_f32<32>), hu_lds()}}, attr_set))
    return false;
  const unsigned grid = (unsigned)(((a.ntiles + HU_XCD - 1) / HU_XCD) * HU_XCD * (Cout / HU_CC));
  const float4* z4 = reinterpret_cast<const float4*>(z);
  float4* o4 = reinterpret_cast<float4*>(out);
  if (Cout == 64) hipLaunchKernelGGL((k_head_upconv_gather_f32<64>), dim3(grid), dim3(HU_NT), hu_lds(), s, z4, o4, a);
  else hipLaunchKernelGGL((k_head_upconv_gather_f32<32>), dim3(grid), dim3(HU_NT), hu_lds(), s, z4, o4, a);
  return true;
}
