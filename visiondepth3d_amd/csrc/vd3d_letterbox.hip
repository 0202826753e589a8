// vd3d_letterbox.hip -- the letterbox handling of the depth pass (core/render_depth.py:280-573: LetterboxTracker and what it calls; :1919-1933: the
// bar fill behind the hand-off), batched over the frames of a step, tracker state on the device, no host synchronisation.
//
//   k_lb_rows         one workgroup per frame row: float32 Rec.709 luma into LDS, the row's mean and variance in numpy's PAIRWISE order (leaf
//                     blocks of <= 128 elements on 8-lane groups, one strided accumulator per lane, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7));
//                     the tree above the leaves from a plan table), the HSV saturation sum, the gray plane, the 64-bin gray histogram and the
//                     integer sum |gray_t - gray_(t-1)| (frame 0 against the plane kept in the tracker state)
//   k_lb_frame_*      y.mean() of the whole plane: numpy reduces it as ONE run of H*W elements in buffers of 8192 (a pairwise sum per buffer, a
//                     running sum over the buffers), so the leaves do not follow the rows
//   k_canny_nms       3 x 3 Sobel (replicated border) + squared magnitude + OpenCV's integer direction test on an LDS tile with a 2-pixel halo
//                     -> class map (0 none, 1 weak, 2 strong)
//   k_hy_*            exact hysteresis without a host loop: union-find over the non-zero pixels (atomicMin on the parents), a flag on every
//                     root whose set holds a strong pixel, a resolve pass that writes the edge map and the per-row edge counts.  The edge set
//                     is unique, so every schedule gives the same map.
//   k_lb_track        one thread walks the B frames in order: near-black gate, scene cut (MAD, then the histogram correlation in double),
//                     cooldown, row scan, sanity caps, even-pixel rule, hysteresis / streak / lock state machine
//   k_fill_*          INTER_CUBIC squeeze of the depth plane into the picture rows (vd3d_cubic.h), 256-bin histogram, int(np.median), bar fill
//
// Arithmetic: one rounding per numpy operator (-ffp-contract=off); the sums that numpy forms exactly are integers here.
#include "vd3d_dev.h"
#include "vd3d_kernels.h"
#include "vd3d_cubic.h"

#include <cstring>
#include <vector>

// ---- numpy's pairwise summation as a plan -------------------------------------------------------------------------------------------
// leaves [nleaf] (offset, length <= 128); combine steps [ncomb] (dst, a, b, 0) over value slots (leaf i = slot i), sorted by height so that the
// steps of one level are independent; level_start [nlevel + 1].  The root is the last slot.
struct vd_pw_plan { int nleaf, ncomb, nlevel, nslot; const int2* leaves; const int4* comb; const int* level_start; };

struct pw_host_plan { std::vector<int2> leaves; std::vector<int4> comb; std::vector<int> level_start; };

static int pw_build_rec(long long lo, long long n, std::vector<int2>& leaves, std::vector<int4>& comb, std::vector<int>& height) {
  if (n <= 128) { leaves.push_back(make_int2((int)lo, (int)n)); return -(int)leaves.size(); }
  long long n2 = n / 2;
  n2 -= n2 % 8;
  const int a = pw_build_rec(lo, n2, leaves, comb, height), b = pw_build_rec(lo + n2, n - n2, leaves, comb, height);
  const int ha = a < 0 ? 0 : height[a], hb = b < 0 ? 0 : height[b];
  comb.push_back(make_int4((int)comb.size(), a, b, 0));
  height.push_back(1 + (ha > hb ? ha : hb));
  return (int)comb.size() - 1;
}

static pw_host_plan pw_build(long long n) {
  pw_host_plan p;
  std::vector<int4> comb;
  std::vector<int> height;
  pw_build_rec(0, n, p.leaves, comb, height);
  const int nl = (int)p.leaves.size();
  int maxh = 0;
  for (int h : height) maxh = h > maxh ? h : maxh;
  p.level_start.assign(1, 0);
  for (int lv = 1; lv <= maxh; ++lv) {
    for (size_t k = 0; k < comb.size(); ++k)
      if (height[k] == lv) {
        const int4 c = comb[k];
        p.comb.push_back(make_int4(nl + c.x, c.y < 0 ? -c.y - 1 : nl + c.y, c.z < 0 ? -c.z - 1 : nl + c.z, 0));
      }
    p.level_start.push_back((int)p.comb.size());
  }
  return p;   // the root keeps the last slot (it is the last step built), whatever its place in the level order
}

struct pw_dev_plan { long long n = 0; int* buf = nullptr; vd_pw_plan p{}; };

// The plan of a length, built and uploaded (blocking copies) the first time a context meets that length and kept until the context goes.  Nothing
// is ever evicted or overwritten -- a queued kernel, or an earlier pw_get of the same call, may hold pointers into any plan -- and the cache is
// bounded by construction: lengths are rows, columns and reduction buffers, all <= 8192 elements, each plan at most ~2.6 KB.
static hipError_t pw_get(std::vector<pw_dev_plan>* cache, long long n, hipStream_t s, vd_pw_plan* out) {
  for (const pw_dev_plan& d : *cache) if (d.n == n) { *out = d.p; return hipSuccess; }
  pw_dev_plan d;
  const pw_host_plan h = pw_build(n);
  const size_t nl = h.leaves.size(), nc = h.comb.size(), nv = h.level_start.size();
  const size_t words = 2 * nl + 4 * (nc ? nc : 1) + nv + 8;
  hipError_t e = hipMalloc((void**)&d.buf, words * sizeof(int));
  if (e != hipSuccess) return e;
  int* comb = d.buf;                        // int4: 16-byte aligned at the head of the allocation
  int* leaves = comb + 4 * (nc ? nc : 1);   // int2
  int* levels = leaves + 2 * nl;
  if (nc) e = hipMemcpy(comb, h.comb.data(), nc * sizeof(int4), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(leaves, h.leaves.data(), nl * sizeof(int2), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(levels, h.level_start.data(), nv * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(d.buf); return e; }
  d.n = n;
  d.p.nleaf = (int)nl; d.p.ncomb = (int)nc; d.p.nlevel = (int)nv - 1; d.p.nslot = (int)(nl + nc);
  d.p.leaves = reinterpret_cast<const int2*>(leaves); d.p.comb = reinterpret_cast<const int4*>(comb); d.p.level_start = levels;
  cache->push_back(d);
  *out = d.p;
  return hipSuccess;
}

// one leaf on an 8-lane group (j = lane & 7; the 8 lanes of a group take the same path): the value is valid in every lane of the group
template <class F>
VD_DEV float pw_leaf8(int n, int j, F val) {
  if (n < 8) {
    float res = 0.f;
    for (int i = 0; i < n; ++i) res = res + val(i);
    return res;
  }
  const int nb = n - (n & 7);
  float acc = val(j);
  for (int i = 8; i < nb; i += 8) acc = acc + val(i + j);
  float t = acc + __shfl_xor(acc, 1, 64);     // r0+r1 | r2+r3 | r4+r5 | r6+r7 (float addition commutes: both lanes of a pair hold the same bits)
  t = t + __shfl_xor(t, 2, 64);
  t = t + __shfl_xor(t, 4, 64);
  for (int i = nb; i < n; ++i) t = t + val(i);
  return t;
}

// the tree above the leaves, level by level, by the whole workgroup; slots in LDS or in global memory
VD_DEV void pw_combine(float* slots, const vd_pw_plan& p) {
  for (int lv = 0; lv < p.nlevel; ++lv) {
    __syncthreads();
    const int k1 = p.level_start[lv + 1];
    for (int k = p.level_start[lv] + (int)threadIdx.x; k < k1; k += (int)blockDim.x) {
      const int4 c = p.comb[k];
      slots[c.x] = slots[c.y] + slots[c.z];
    }
  }
  __syncthreads();
}

// ---- colour ---------------------------------------------------------------------------------------------------------------------------
VD_DEV float lb_luma(const uint8_t* p) { return (0.2126f * (float)p[2] + 0.7152f * (float)p[1]) + 0.0722f * (float)p[0]; }
VD_DEV int lb_gray(const uint8_t* p) { return ((int)p[0] * 1868 + (int)p[1] * 9617 + (int)p[2] * 4899 + 8192) >> 14; }

// tracker state in device memory: the exported scalars, then what the next batch compares its first frame with
struct vd_lb_state { vd3d_letterbox_state s; uint32_t prev_hist[64]; };

#define LB_MAX_W 8192
#define LB_MAX_LEAVES 256   // slots of a row plan: W <= 8192 gives at most 65 leaves + 64 steps (lengths 7689 .. 8191 split finer than 8192 does)

struct vd_lb_rows_args { int B, H, W, chain; };

__global__ __launch_bounds__(256) void k_lb_rows(const uint8_t* __restrict__ frames, vd_lb_rows_args a, vd_pw_plan plan, const vd_lb_state* __restrict__ st,
                                                 const uint8_t* __restrict__ st_gray, float* __restrict__ row_mean, float* __restrict__ row_var,
                                                 uint32_t* __restrict__ row_sat, uint8_t* __restrict__ gray, uint32_t* __restrict__ hist,
                                                 unsigned long long* __restrict__ mad) {
  extern __shared__ float sy[];                 // [W] luma, then (y - mean)^2
  __shared__ float slots[LB_MAX_LEAVES];
  __shared__ int sdiv[256];
  __shared__ uint32_t lhist[64];
  __shared__ uint32_t s_sat, s_mad;
  const int y = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t row = ((size_t)b * a.H + y) * a.W;
  const uint8_t* src = frames + row * 3;
  // the frame before: inside the batch its pixels (the gray value is recomputed), for frame 0 the plane in the tracker state
  const uint8_t* prev_px = b > 0 ? src - (size_t)a.H * a.W * 3 : nullptr;
  const uint8_t* prev_g = nullptr;
  if (b == 0 && a.chain && st->s.have_prev && st->s.prev_h == a.H && st->s.prev_w == a.W) prev_g = st_gray + (size_t)y * a.W;
  sdiv[tid] = tid ? (int)rint(1044480.0 / (double)tid) : 0;   // round((255 << 12) / v)
  if (tid < 64) lhist[tid] = 0u;
  if (tid == 0) { s_sat = 0u; s_mad = 0u; }
  __syncthreads();
  uint32_t sat = 0u, md = 0u;
  for (int x = tid; x < a.W; x += 256) {
    const uint8_t* p = src + 3 * x;
    sy[x] = lb_luma(p);
    const int g = lb_gray(p);
    gray[row + x] = (uint8_t)g;
    atomicAdd(&lhist[g >> 2], 1u);
    const int v = max(max((int)p[0], (int)p[1]), (int)p[2]), mn = min(min((int)p[0], (int)p[1]), (int)p[2]);
    sat += (uint32_t)(((v - mn) * sdiv[v] + 2048) >> 12);
    if (prev_px) md += (uint32_t)abs(g - lb_gray(prev_px + 3 * x));
    else if (prev_g) md += (uint32_t)abs(g - (int)prev_g[x]);
  }
  atomicAdd(&s_sat, sat);
  atomicAdd(&s_mad, md);
  __syncthreads();
  const int grp = tid >> 3, j = tid & 7;
  float mean = 0.f;
  for (int pass = 0; pass < 2; ++pass) {
    for (int l0 = 0; l0 < plan.nleaf; l0 += 32) {
      const int l = l0 + grp;
      if (l < plan.nleaf) {
        const int2 lf = plan.leaves[l];
        const float* base = sy + lf.x;
        const float v = pw_leaf8(lf.y, j, [&](int i) { return base[i]; });
        if (j == 0) slots[l] = v;
      }
    }
    pw_combine(slots, plan);
    const float sum = slots[plan.nslot - 1];
    if (pass == 0) {
      mean = sum / (float)a.W;
      __syncthreads();
      for (int x = tid; x < a.W; x += 256) { const float d = sy[x] - mean; sy[x] = d * d; }
      __syncthreads();
    } else if (tid == 0) {
      row_mean[(size_t)b * a.H + y] = mean;
      row_var[(size_t)b * a.H + y] = sum / (float)a.W;
      row_sat[(size_t)b * a.H + y] = s_sat;
      if (s_mad) atomicAdd(&mad[b], (unsigned long long)s_mad);
    }
  }
  if (tid < 64 && lhist[tid]) atomicAdd(&hist[(size_t)b * 64 + tid], lhist[tid]);
}

// whole-frame luma mean.  numpy reduces the contiguous plane as one run of H*W elements, but through its 8192-element iteration buffer: every
// chunk of LB_CHUNK elements is a pairwise sum of its own and the chunk sums are added up one after the other.  Leaves: 32 per workgroup.
#define LB_CHUNK 8192
struct vd_lb_frame_args { long long n; int nchunk, nfull, nslot; };   // nfull chunks of LB_CHUNK elements, then (nchunk - nfull) = 0 or 1 shorter one

__global__ __launch_bounds__(256) void k_lb_frame_leaves(const uint8_t* __restrict__ frames, vd_lb_frame_args a, vd_pw_plan full, vd_pw_plan tail,
                                                         float* __restrict__ slots) {
  const int c = blockIdx.y, b = blockIdx.z;
  const vd_pw_plan& plan = c < a.nfull ? full : tail;
  const int l = blockIdx.x * 32 + (threadIdx.x >> 3), j = threadIdx.x & 7;
  if (l >= plan.nleaf) return;
  const int2 lf = plan.leaves[l];
  const uint8_t* base = frames + ((size_t)b * (size_t)a.n + (size_t)c * LB_CHUNK + (size_t)lf.x) * 3;
  const float v = pw_leaf8(lf.y, j, [&](int i) { return lb_luma(base + 3 * i); });
  if (j == 0) slots[((size_t)b * a.nchunk + c) * a.nslot + l] = v;
}

__global__ __launch_bounds__(128) void k_lb_frame_combine(vd_lb_frame_args a, vd_pw_plan full, vd_pw_plan tail, float* __restrict__ slots, float* __restrict__ csum) {
  const int c = blockIdx.x, b = blockIdx.y;
  const vd_pw_plan& plan = c < a.nfull ? full : tail;
  float* s = slots + ((size_t)b * a.nchunk + c) * a.nslot;
  pw_combine(s, plan);
  if (threadIdx.x == 0) csum[(size_t)b * a.nchunk + c] = s[plan.nslot - 1];
}

__global__ __launch_bounds__(256) void k_lb_frame_mean(vd_lb_frame_args a, const float* __restrict__ csum, float* __restrict__ fmean) {
  __shared__ float part[1024];
  const float* src = csum + (size_t)blockIdx.x * a.nchunk;
  float acc = 0.f;
  for (int c0 = 0; c0 < a.nchunk; c0 += 1024) {
    const int m = min(1024, a.nchunk - c0);
    for (int i = threadIdx.x; i < m; i += 256) part[i] = src[c0 + i];
    __syncthreads();
    if (threadIdx.x == 0) for (int i = 0; i < m; ++i) acc = acc + part[i];   // in order: numpy's running sum over its buffers
    __syncthreads();
  }
  if (threadIdx.x == 0) fmean[blockIdx.x] = acc / (float)a.n;
}

// ---- Canny: Sobel + magnitude + non-maximum test -----------------------------------------------------------------------------------------
#define CN_TW 64
#define CN_TH 16
__global__ __launch_bounds__(256) void k_canny_nms(const uint8_t* __restrict__ gray, int H, int W, int low2, int high2, uint8_t* __restrict__ cls) {
  __shared__ uint8_t g[CN_TH + 4][CN_TW + 4];
  __shared__ int mag[CN_TH + 2][CN_TW + 2];
  const int x0 = blockIdx.x * CN_TW, y0 = blockIdx.y * CN_TH, b = blockIdx.z, tid = threadIdx.x;
  const uint8_t* src = gray + (size_t)b * H * W;
  for (int i = tid; i < (CN_TH + 4) * (CN_TW + 4); i += 256) {
    const int ly = i / (CN_TW + 4), lx = i - ly * (CN_TW + 4);
    const int yy = min(max(y0 + ly - 2, 0), H - 1), xx = min(max(x0 + lx - 2, 0), W - 1);   // replicated border
    g[ly][lx] = src[(size_t)yy * W + xx];
  }
  __syncthreads();
  // gradient at local (ly, lx) of the magnitude tile = image (y0 + ly - 1, x0 + lx - 1) = gray tile (ly + 1, lx + 1)
  auto grad = [&](int ly, int lx, int* dx, int* dy) {
    const int gy = ly + 1, gx = lx + 1;
    const int a00 = g[gy - 1][gx - 1], a01 = g[gy - 1][gx], a02 = g[gy - 1][gx + 1], a10 = g[gy][gx - 1], a12 = g[gy][gx + 1];
    const int a20 = g[gy + 1][gx - 1], a21 = g[gy + 1][gx], a22 = g[gy + 1][gx + 1];
    *dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
    *dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
  };
  for (int i = tid; i < (CN_TH + 2) * (CN_TW + 2); i += 256) {
    const int ly = i / (CN_TW + 2), lx = i - ly * (CN_TW + 2);
    const int yy = y0 + ly - 1, xx = x0 + lx - 1;
    int m = 0;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) { int dx, dy; grad(ly, lx, &dx, &dy); m = dx * dx + dy * dy; }   // 0 outside the image
    mag[ly][lx] = m;
  }
  __syncthreads();
  const int lx = tid & 63;
  for (int r = tid >> 6; r < CN_TH; r += 4) {
    const int yy = y0 + r, xx = x0 + lx;
    if (yy >= H || xx >= W) continue;
    const int my = r + 1, mx = lx + 1, m = mag[my][mx];
    int c = 0;
    if (m > low2) {
      int dx, dy;
      grad(my, mx, &dx, &dy);
      const int ax = abs(dx), ay = abs(dy) << 15, t = 13573 * ax;
      bool keep;
      if (ay < t) keep = m > mag[my][mx - 1] && m >= mag[my][mx + 1];
      else if (ay > t + (ax << 16)) keep = m > mag[my - 1][mx] && m >= mag[my + 1][mx];
      else { const int s = (dx ^ dy) < 0 ? -1 : 1; keep = m > mag[my - 1][mx - s] && m > mag[my + 1][mx + s]; }
      if (keep) c = m > high2 ? 2 : 1;
    }
    cls[((size_t)b * H + yy) * W + xx] = (uint8_t)c;
  }
}

// ---- hysteresis: union-find over the non-zero pixels of a class map ------------------------------------------------------------------
// Parents only ever decrease (atomicMin) and every link goes through an atomic on the true value, so a stale plain read in hy_find can only
// return an older ancestor of the same set: the result does not depend on the schedule.
VD_DEV int hy_find(const int* L, int x) {
  int p = L[x];
  while (p != x) { x = p; p = L[x]; }
  return x;
}
// ... while other workgroups link: relaxed atomic loads, so that the compiler re-reads a parent after every atomicMin
VD_DEV int hy_find_live(int* L, int x) {
  int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) { x = p; p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  return x;
}
VD_DEV void hy_union(int* L, int a, int b) {
  while (true) {
    a = hy_find_live(L, a); b = hy_find_live(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }   // a > b: hang a under b
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;                                         // a had a parent already: go on with it (b is merged with that set next)
  }
}

__global__ __launch_bounds__(256) void k_hy_init(const uint8_t* __restrict__ cls, long long n, int* __restrict__ L, uint8_t* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const size_t o = (size_t)blockIdx.y * (size_t)n;
  if (i < n) { L[o + i] = cls[o + i] ? (int)i : -1; flag[o + i] = 0; }
}
__global__ __launch_bounds__(256) void k_hy_merge(const uint8_t* __restrict__ cls, int H, int W, int* __restrict__ L) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t o = (size_t)blockIdx.z * H * W;
  const uint8_t* c = cls + o;
  int* l = L + o;
  const int i = y * W + x;
  if (!c[i]) return;
  // the four forward neighbours of the 8-neighbourhood: every adjacent pair is visited once
  if (x + 1 < W && c[i + 1]) hy_union(l, i, i + 1);
  if (y + 1 < H) {
    if (x > 0 && c[i + W - 1]) hy_union(l, i, i + W - 1);
    if (c[i + W]) hy_union(l, i, i + W);
    if (x + 1 < W && c[i + W + 1]) hy_union(l, i, i + W + 1);
  }
}
__global__ __launch_bounds__(256) void k_hy_flag(const uint8_t* __restrict__ cls, long long n, int* __restrict__ L, uint8_t* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const size_t o = (size_t)blockIdx.y * (size_t)n;
  if (i >= n || !cls[o + i]) return;
  const int r = hy_find(L + o, (int)i);
  L[o + i] = r;                          // a root or an ancestor either way: concurrent finds stay correct
  if (cls[o + i] >= 2) flag[o + r] = 1;  // every writer stores the same value
}
__global__ __launch_bounds__(256) void k_hy_resolve(const uint8_t* __restrict__ cls, int H, int W, const int* __restrict__ L, const uint8_t* __restrict__ flag,
                                                    uint8_t* __restrict__ edges, int* __restrict__ rowcnt) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const size_t o = (size_t)blockIdx.z * H * W;
  bool e = false;
  if (x < W) {
    const int i = y * W + x;
    if (cls[o + i]) e = flag[o + hy_find(L + o, i)] != 0;
    edges[o + i] = e ? 255 : 0;
  }
  if (rowcnt) {
    const unsigned long long m = __ballot(e);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&rowcnt[(size_t)blockIdx.z * H + y], __popcll(m));
  }
}

// ---- tracker step -------------------------------------------------------------------------------------------------------------------------
struct vd_lb_track_args { int B, H, W, scan_h, min_band, min_change, confirm_needed, max_total, cooldown_frames; };

// pairwise float64 sum of e[i] = ((255 * count[i]) / W) / 255.0 over the H rows, by one thread: leaves with 8 accumulators, then the plan's steps
VD_DEV double lb_edge_mean(const int* __restrict__ cnt, int H, int W, const vd_pw_plan& p, double* slots) {
  const double w = (double)W;
  auto val = [&](int i) { return ((255.0 * (double)cnt[i]) / w) / 255.0; };
  for (int l = 0; l < p.nleaf; ++l) {
    const int2 lf = p.leaves[l];
    const int n = lf.y, o = lf.x;
    double res;
    if (n < 8) { res = 0.0; for (int i = 0; i < n; ++i) res = res + val(o + i); }
    else {
      double r[8];
      for (int j = 0; j < 8; ++j) r[j] = val(o + j);
      int i = 8;
      for (; i < n - (n & 7); i += 8) for (int j = 0; j < 8; ++j) r[j] = r[j] + val(o + i + j);
      res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (; i < n; ++i) res = res + val(o + i);
    }
    slots[l] = res;
  }
  for (int k = 0; k < p.ncomb; ++k) { const int4 c = p.comb[k]; slots[c.x] = slots[c.y] + slots[c.z]; }   // by level: children first
  return slots[p.nslot - 1] / (double)H;
}

// cv2.normalize (L2) of both histograms, then compareHist(HISTCMP_CORREL): the statement's float64 order
VD_DEV double lb_hist_correl(const uint32_t* __restrict__ h1, const uint32_t* __restrict__ h2) {
  double n1 = 0.0, n2 = 0.0;
  for (int i = 0; i < 64; ++i) { n1 += (double)h1[i] * (double)h1[i]; n2 += (double)h2[i] * (double)h2[i]; }   // exact integers
  n1 = sqrt(n1); n2 = sqrt(n2);
  const double eps = 2.220446049250313e-16;
  const double sc1 = n1 > eps ? 1.0 / n1 : 0.0, sc2 = n2 > eps ? 1.0 / n2 : 0.0;
  double s1 = 0.0, s2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
  for (int i = 0; i < 64; ++i) {
    const double x = (double)(float)((double)h1[i] * sc1), y = (double)(float)((double)h2[i] * sc2);
    s1 += x; s2 += y; s11 += x * x; s22 += y * y; s12 += x * y;
  }
  const double scale = 1.0 / 64.0;
  const double num = s12 - s1 * s2 * scale, den2 = (s11 - s1 * s1 * scale) * (s22 - s2 * s2 * scale);
  return fabs(den2) > eps ? num / sqrt(den2) : 1.0;
}

__global__ __launch_bounds__(64) void k_lb_track(vd_lb_track_args a, vd_pw_plan hplan, vd_lb_state* __restrict__ st, const float* __restrict__ row_mean,
                                                 const float* __restrict__ row_var, const uint32_t* __restrict__ row_sat, const uint32_t* __restrict__ hist,
                                                 const unsigned long long* __restrict__ mad, const float* __restrict__ fmean,
                                                 const int* __restrict__ rowcnt, double* __restrict__ slots, int32_t* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  vd3d_letterbox_state s = st->s;
  for (int b = 0; b < a.B; ++b) {
    const size_t r0 = (size_t)b * a.H;
    if (s.cooldown > 0) s.cooldown--;
    const double emean = lb_edge_mean(rowcnt + r0, a.H, a.W, hplan, slots);
    const bool black = (double)fmean[b] < 18.0 && emean < 0.02;
    bool cut = false;
    if (!black) {
      const bool have = b > 0 || s.have_prev;
      if (have) {
        if (b == 0 && (s.prev_h != a.H || s.prev_w != a.W)) cut = true;
        else {
          const double m = (double)mad[b] / (double)((long long)a.H * a.W);
          if (m > 28.0) cut = true;
          else cut = lb_hist_correl(b ? hist + (size_t)(b - 1) * 64 : st->prev_hist, hist + (size_t)b * 64) < 0.60;
        }
      }
    }
    if (cut && s.cooldown <= 0) {
      int mt = 0, mb = 0;
      if (a.H >= 64 && a.W >= 64) {
        const float w = (float)a.W;
        const double dw = (double)a.W;
        auto ok = [&](int i) {
          return row_mean[r0 + i] < 16.0f && row_var[r0 + i] < 3.0f && (float)row_sat[r0 + i] / w < 6.0f &&
                 ((255.0 * (double)rowcnt[r0 + i]) / dw) / 255.0 <= 0.04;
        };
        for (int i = 0; i < a.scan_h && ok(i); ++i) ++mt;
        for (int i = a.H - 1; i > a.H - 1 - a.scan_h && ok(i); --i) ++mb;
        if (mt < a.min_band) mt = 0;
        if (mb < a.min_band) mb = 0;
        mt -= mt & 1; mb -= mb & 1;
        if ((double)(mt + mb) >= (double)a.H * 0.6) { mt = 0; mb = 0; }
      }
      if (mt + mb > a.max_total) { mt = 0; mb = 0; }
      const int change = abs(mt - s.top) + abs(mb - s.bottom);
      if (change < a.min_change) { s.streak = 0; s.cand_top = s.top; s.cand_bottom = s.bottom; }
      else {
        if (mt == s.cand_top && mb == s.cand_bottom) s.streak++;
        else { s.cand_top = mt; s.cand_bottom = mb; s.streak = 1; }
        if (s.streak >= a.confirm_needed) {
          if (s.locked_zero && mt + mb > 0) { s.top = mt; s.bottom = mb; s.locked_zero = 0; s.locked_bars = 1; s.cooldown = a.cooldown_frames; }
          else if (s.locked_bars) { s.top = mt; s.bottom = mb; s.locked_zero = mt + mb == 0; s.locked_bars = mt + mb > 0; s.cooldown = a.cooldown_frames; }
        }
      }
    }
    out[2 * b] = s.top; out[2 * b + 1] = s.bottom;
  }
  st->s = s;
}

// after a chained batch: the last frame's histogram (its gray plane follows by a device copy) is what the next batch compares with
__global__ __launch_bounds__(64) void k_lb_commit(vd_lb_state* __restrict__ st, const uint32_t* __restrict__ hist_last, int H, int W) {
  st->prev_hist[threadIdx.x] = hist_last[threadIdx.x];
  if (threadIdx.x == 0) { st->s.have_prev = 1; st->s.prev_h = H; st->s.prev_w = W; }
}

// ---- bar fill ----------------------------------------------------------------------------------------------------------------------------
// (top, bottom) of frame b as the reference uses them: negative values count as 0; bars that leave no picture row are dropped
VD_DEV void fill_geometry(const int32_t* __restrict__ bars, int stride, int b, int H, int* top, int* core_h, bool* copy) {
  int t = bars[(size_t)b * stride], bo = bars[(size_t)b * stride + 1];
  t = t < 0 ? 0 : (t > H ? H : t); bo = bo < 0 ? 0 : (bo > H ? H : bo);
  *copy = (t == 0 && bo == 0) || H - t - bo <= 0;
  *top = *copy ? 0 : t;
  *core_h = *copy ? H : H - t - bo;
}

__global__ __launch_bounds__(256) void k_fill_squeeze(const uint8_t* __restrict__ depth, int H, int W, const int32_t* __restrict__ bars, int stride,
                                                      uint8_t* __restrict__ out, uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[256];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  int top, core_h; bool copy;
  fill_geometry(bars, stride, b, H, &top, &core_h, &copy);
  lh[threadIdx.x] = 0u;
  __syncthreads();
  const uint8_t* src = depth + (size_t)b * H * W;
  if (x < W && r < core_h) {
    uint8_t v;
    if (copy) v = src[(size_t)r * W + x];
    else {   // cv2.resize(depth, (W, core_h), INTER_CUBIC): the width is kept (identity taps), the rows are squeezed
      const rc_axis ax = rc_axis_make(x, 1.0, W), ay = rc_axis_make(r, 1.0 / ((double)core_h / (double)H), H);
      rc_cubic_pixel<1>(src, (size_t)W, ax, ay, &v);
      atomicAdd(&lh[v], 1u);
    }
    out[((size_t)b * H + top + r) * W + x] = v;
  }
  __syncthreads();
  if (!copy && lh[threadIdx.x]) atomicAdd(&hist[(size_t)b * 256 + threadIdx.x], lh[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_fill_bars(int H, int W, const int32_t* __restrict__ bars, int stride, const uint32_t* __restrict__ hist,
                                                   uint8_t* __restrict__ out) {
  __shared__ int s_med;
  const int b = blockIdx.z;
  int top, core_h; bool copy;
  fill_geometry(bars, stride, b, H, &top, &core_h, &copy);
  if (copy) return;
  const int nbar = H - core_h;
  const int r = blockIdx.y * 4 + (threadIdx.x >> 6), x = blockIdx.x * 64 + (threadIdx.x & 63);
  if (blockIdx.y * 4 >= nbar) return;
  if (threadIdx.x == 0) {   // int(np.median): the middle value, or the truncated mean of the two middle values
    const long long n = (long long)core_h * W, k1 = n / 2, k0 = (n & 1) ? k1 : k1 - 1;
    long long acc = 0;
    int v0 = -1, v1 = 0;
    for (int v = 0; v < 256; ++v) {
      acc += hist[(size_t)b * 256 + v];
      if (v0 < 0 && acc > k0) v0 = v;
      if (acc > k1) { v1 = v; break; }
    }
    s_med = (v0 + v1) >> 1;
  }
  __syncthreads();
  if (r < nbar && x < W) {
    const int y = r < top ? r : core_h + r;   // rows above the picture, then the rows below it
    out[((size_t)b * H + y) * W + x] = (uint8_t)s_med;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// every buffer has its own capacity and grows through lb_grow alone
template <class T> struct lb_buf { T* p = nullptr; size_t cap = 0; };

struct vd_lb_ws {
  vd_lb_state* st = nullptr;
  std::vector<pw_dev_plan> plans;
  lb_buf<uint8_t> st_gray, flag, cls, gray, edges;
  lb_buf<float> fslots, row_mean, row_var, fmean;
  lb_buf<double> dslots;
  lb_buf<int> L, rowcnt;
  lb_buf<uint32_t> row_sat, hist, fill_hist;
  lb_buf<unsigned long long> mad;
};

#define LBCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

template <class T> static hipError_t lb_grow(lb_buf<T>* b, size_t n, hipStream_t s) {
  if (n <= b->cap && b->p) return hipSuccess;
  if (b->p) {   // queued kernels may still use the old buffer
    LBCHK(hipStreamSynchronize(s));
    T* old = b->p;
    b->p = nullptr; b->cap = 0;
    LBCHK(hipFree(old));
  }
  LBCHK(hipMalloc((void**)&b->p, n * sizeof(T)));
  b->cap = n;
  return hipSuccess;
}

__global__ void k_lb_reset(vd_lb_state* st) {   // a new tracker: the reference's default is "no bars" (locked_zero), nothing kept
  const int i = threadIdx.x;
  int32_t* w = reinterpret_cast<int32_t*>(&st->s);
  if (i < (int)(sizeof(vd3d_letterbox_state) / sizeof(int32_t))) w[i] = 0;
  if (i < 64) st->prev_hist[i] = 0u;
  __syncthreads();
  if (i == 0) st->s.locked_zero = 1;
}

static hipError_t lb_ws(vd_lb_ws** pws, hipStream_t s) {
  if (*pws) return hipSuccess;
  vd_lb_ws* w = new vd_lb_ws();
  const hipError_t e = hipMalloc((void**)&w->st, sizeof(vd_lb_state));
  if (e != hipSuccess) { delete w; return e; }
  *pws = w;
  hipLaunchKernelGGL(k_lb_reset, dim3(1), dim3(64), 0, s, w->st);
  return hipGetLastError();
}

void vd_lb_free(vd_lb_ws* w) {
  if (!w) return;
  void* ptrs[] = {w->st, w->st_gray.p, w->flag.p, w->cls.p, w->gray.p, w->edges.p, w->fslots.p, w->row_mean.p, w->row_var.p, w->fmean.p, w->dslots.p,
                  w->L.p, w->rowcnt.p, w->row_sat.p, w->hist.p, w->fill_hist.p, w->mad.p};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  for (const pw_dev_plan& d : w->plans) (void)hipFree(d.buf);
  delete w;
}

hipError_t vd_lb_state_reset(vd_lb_ws** pws, hipStream_t s) {
  LBCHK(lb_ws(pws, s));
  hipLaunchKernelGGL(k_lb_reset, dim3(1), dim3(64), 0, s, (*pws)->st);
  return hipGetLastError();
}

hipError_t vd_lb_state_export(vd_lb_ws** pws, hipStream_t s, vd3d_letterbox_state* out, uint32_t* prev_hist64, uint8_t* prev_gray_dev, long long gray_cap) {
  LBCHK(lb_ws(pws, s));
  vd_lb_ws* w = *pws;
  vd_lb_state h;
  LBCHK(hipMemcpyAsync(&h, w->st, sizeof h, hipMemcpyDeviceToHost, s));
  LBCHK(hipStreamSynchronize(s));
  *out = h.s;
  if (prev_hist64) memcpy(prev_hist64, h.prev_hist, sizeof h.prev_hist);
  if (prev_gray_dev && h.s.have_prev) {
    const long long n = (long long)h.s.prev_h * h.s.prev_w;
    if (n > gray_cap || (size_t)n > w->st_gray.cap) return hipErrorInvalidValue;
    LBCHK(hipMemcpyAsync(prev_gray_dev, w->st_gray.p, (size_t)n, hipMemcpyDeviceToDevice, s));
  }
  return hipSuccess;
}

hipError_t vd_lb_state_import(vd_lb_ws** pws, hipStream_t s, const vd3d_letterbox_state* in, const uint32_t* prev_hist64, const uint8_t* prev_gray_dev) {
  LBCHK(lb_ws(pws, s));
  vd_lb_ws* w = *pws;
  vd_lb_state h;
  memset(&h, 0, sizeof h);
  h.s = *in;
  if (!prev_hist64 || !prev_gray_dev || h.s.prev_h < 1 || h.s.prev_w < 1) { h.s.have_prev = 0; h.s.prev_h = 0; h.s.prev_w = 0; }
  if (h.s.have_prev) {
    memcpy(h.prev_hist, prev_hist64, sizeof h.prev_hist);
    const size_t n = (size_t)h.s.prev_h * h.s.prev_w;
    LBCHK(lb_grow(&w->st_gray, n, s));
    LBCHK(hipMemcpyAsync(w->st_gray.p, prev_gray_dev, n, hipMemcpyDeviceToDevice, s));
  }
  LBCHK(hipMemcpyAsync(w->st, &h, sizeof h, hipMemcpyHostToDevice, s));
  return hipStreamSynchronize(s);   // `h` is on this stack frame
}

// W and H within one of numpy's 8192-element reduction buffers: a row, and the column of row densities, are each ONE pairwise sum
bool vd_lb_size_ok(int B, int H, int W) { return B <= 4096 && H <= 8192 && W <= LB_MAX_W; }

hipError_t vd_lb_stats(vd_lb_ws** pws, hipStream_t s, const uint8_t* frames, int B, int H, int W, int chain, float* row_mean, float* row_var,
                       uint32_t* row_sat, uint8_t* gray, uint32_t* hist, unsigned long long* mad, float* fmean) {
  LBCHK(lb_ws(pws, s));
  vd_lb_ws* w = *pws;
  const long long n = (long long)H * W;
  vd_pw_plan plan_w, plan_c, plan_t;   // a row, a full chunk of the plane, its last chunk
  LBCHK(pw_get(&w->plans, W, s, &plan_w));
  vd_lb_frame_args fa;
  fa.n = n; fa.nfull = (int)(n / LB_CHUNK); fa.nchunk = (int)((n + LB_CHUNK - 1) / LB_CHUNK);
  LBCHK(pw_get(&w->plans, LB_CHUNK, s, &plan_c));
  LBCHK(pw_get(&w->plans, fa.nchunk > fa.nfull ? n - (long long)fa.nfull * LB_CHUNK : LB_CHUNK, s, &plan_t));
  // A shorter last chunk can have MORE leaves than a full one (8192 elements split into 64 leaves of 128; 8100 into 65 of 120 - 128): the slot
  // stride and the leaf grid take the larger of the two plans
  fa.nslot = plan_c.nslot > plan_t.nslot ? plan_c.nslot : plan_t.nslot;
  const int nleaf = plan_c.nleaf > plan_t.nleaf ? plan_c.nleaf : plan_t.nleaf;
  const size_t nsl = (size_t)B * fa.nchunk * fa.nslot;
  LBCHK(lb_grow(&w->fslots, nsl + (size_t)B * fa.nchunk, s));
  float* csum = w->fslots.p + nsl;
  if (chain) LBCHK(lb_grow(&w->st_gray, (size_t)n, s));
  LBCHK(hipMemsetAsync(hist, 0, (size_t)B * 64 * sizeof(uint32_t), s));
  LBCHK(hipMemsetAsync(mad, 0, (size_t)B * sizeof(unsigned long long), s));
  vd_lb_rows_args a;
  a.B = B; a.H = H; a.W = W; a.chain = chain ? 1 : 0;
  hipLaunchKernelGGL(k_lb_rows, dim3(H, B), dim3(256), (size_t)W * sizeof(float), s, frames, a, plan_w, w->st, w->st_gray.p, row_mean, row_var, row_sat,
                     gray, hist, mad);
  hipLaunchKernelGGL(k_lb_frame_leaves, dim3((nleaf + 31) / 32, fa.nchunk, B), dim3(256), 0, s, frames, fa, plan_c, plan_t, w->fslots.p);
  hipLaunchKernelGGL(k_lb_frame_combine, dim3(fa.nchunk, B), dim3(128), 0, s, fa, plan_c, plan_t, w->fslots.p, csum);
  hipLaunchKernelGGL(k_lb_frame_mean, dim3(B), dim3(256), 0, s, fa, csum, fmean);
  return hipGetLastError();
}

// the last frame of a chained batch becomes the state's previous frame
static hipError_t lb_commit(vd_lb_ws* w, hipStream_t s, const uint8_t* gray, const uint32_t* hist, int B, int H, int W) {
  const size_t n = (size_t)H * W;
  LBCHK(hipMemcpyAsync(w->st_gray.p, gray + (size_t)(B - 1) * n, n, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_lb_commit, dim3(1), dim3(64), 0, s, w->st, hist + (size_t)(B - 1) * 64, H, W);
  return hipGetLastError();
}

hipError_t vd_lb_stats_commit(vd_lb_ws** pws, hipStream_t s, const uint8_t* gray, const uint32_t* hist, int B, int H, int W) {
  return lb_commit(*pws, s, gray, hist, B, H, W);
}

hipError_t vd_lb_hysteresis(vd_lb_ws** pws, hipStream_t s, const uint8_t* cls, int B, int H, int W, uint8_t* edges, int32_t* rowcnt) {
  LBCHK(lb_ws(pws, s));
  vd_lb_ws* w = *pws;
  const long long n = (long long)H * W;
  const size_t px = (size_t)B * (size_t)n;
  LBCHK(lb_grow(&w->L, px, s));
  LBCHK(lb_grow(&w->flag, px, s));
  if (rowcnt) LBCHK(hipMemsetAsync(rowcnt, 0, (size_t)B * H * sizeof(int32_t), s));
  const dim3 lin((unsigned)((n + 255) / 256), B);
  hipLaunchKernelGGL(k_hy_init, lin, dim3(256), 0, s, cls, n, w->L.p, w->flag.p);
  hipLaunchKernelGGL(k_hy_merge, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(256), 0, s, cls, H, W, w->L.p);
  hipLaunchKernelGGL(k_hy_flag, lin, dim3(256), 0, s, cls, n, w->L.p, w->flag.p);
  hipLaunchKernelGGL(k_hy_resolve, dim3((W + 255) / 256, H, B), dim3(256), 0, s, cls, H, W, w->L.p, w->flag.p, edges, rowcnt);
  return hipGetLastError();
}

hipError_t vd_lb_canny(vd_lb_ws** pws, hipStream_t s, const uint8_t* gray, int B, int H, int W, int low, int high, uint8_t* edges, int32_t* rowcnt) {
  LBCHK(lb_ws(pws, s));
  vd_lb_ws* w = *pws;
  LBCHK(lb_grow(&w->cls, (size_t)B * H * W, s));
  hipLaunchKernelGGL(k_canny_nms, dim3((W + CN_TW - 1) / CN_TW, (H + CN_TH - 1) / CN_TH, B), dim3(256), 0, s, gray, H, W, low * low, high * high, w->cls.p);
  return vd_lb_hysteresis(pws, s, w->cls.p, B, H, W, edges, rowcnt);
}

hipError_t vd_lb_track(vd_lb_ws** pws, hipStream_t s, const uint8_t* frames, int B, int H, int W, const vd3d_letterbox_params* p, int32_t* out_bars) {
  LBCHK(lb_ws(pws, s));
  vd_lb_ws* w = *pws;
  const size_t n = (size_t)H * W, rows = (size_t)B * H;
  LBCHK(lb_grow(&w->gray, (size_t)B * n, s));
  LBCHK(lb_grow(&w->edges, (size_t)B * n, s));
  LBCHK(lb_grow(&w->row_mean, rows, s));
  LBCHK(lb_grow(&w->row_var, rows, s));
  LBCHK(lb_grow(&w->row_sat, rows, s));
  LBCHK(lb_grow(&w->rowcnt, rows, s));
  LBCHK(lb_grow(&w->hist, (size_t)B * 64, s));
  LBCHK(lb_grow(&w->mad, (size_t)B, s));
  LBCHK(lb_grow(&w->fmean, (size_t)B, s));
  vd_pw_plan plan_h;   // the column of row densities
  LBCHK(pw_get(&w->plans, H, s, &plan_h));
  LBCHK(lb_grow(&w->dslots, (size_t)plan_h.nslot, s));
  LBCHK(vd_lb_stats(pws, s, frames, B, H, W, 1, w->row_mean.p, w->row_var.p, w->row_sat.p, w->gray.p, w->hist.p, w->mad.p, w->fmean.p));
  LBCHK(vd_lb_canny(pws, s, w->gray.p, B, H, W, 30, 90, w->edges.p, w->rowcnt.p));
  vd_lb_track_args a;
  a.B = B; a.H = H; a.W = W;
  a.scan_h = (int)((double)H * 0.25); a.min_band = (int)((double)H * 0.06);
  a.min_change = p->min_change; a.confirm_needed = p->confirm_needed; a.max_total = p->max_total; a.cooldown_frames = p->cooldown_frames;
  hipLaunchKernelGGL(k_lb_track, dim3(1), dim3(64), 0, s, a, plan_h, w->st, w->row_mean.p, w->row_var.p, w->row_sat.p, w->hist.p, w->mad.p, w->fmean.p,
                     w->rowcnt.p, w->dslots.p, out_bars);
  return lb_commit(w, s, w->gray.p, w->hist.p, B, H, W);
}

hipError_t vd_lb_fill(vd_lb_ws** pws, hipStream_t s, const uint8_t* depth, int B, int H, int W, const int32_t* bars_dev, int bars_stride, uint8_t* out) {
  LBCHK(lb_ws(pws, s));
  vd_lb_ws* w = *pws;
  LBCHK(lb_grow(&w->fill_hist, (size_t)B * 256, s));
  LBCHK(hipMemsetAsync(w->fill_hist.p, 0, (size_t)B * 256 * sizeof(uint32_t), s));
  const dim3 g((W + 63) / 64, (H + 3) / 4, B);
  hipLaunchKernelGGL(k_fill_squeeze, g, dim3(256), 0, s, depth, H, W, bars_dev, bars_stride, out, w->fill_hist.p);
  hipLaunchKernelGGL(k_fill_bars, g, dim3(256), 0, s, H, W, bars_dev, bars_stride, w->fill_hist.p, out);
  return hipGetLastError();
}
