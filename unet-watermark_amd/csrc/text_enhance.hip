// The reference's text-feature enhancement (WatermarkPredictor._enhance_text_features, src/predict.py:370-404) on the device, for a
// ragged batch of uint8 RGB images at their own sizes.  include/uwm.h and DESIGN.md §8n are the specification:
//   grey (cv2's 8-bit RGB2GRAY)  ->  CLAHE(2.0, 8 x 8 tiles, cv2's padding rule)  ->  Canny(50, 150), aperture 3, L1 magnitude  ->
//   dilate with the 2 x 2 ellipse  ->  x 1.2 on the channels of the dilated-edge pixels  ->  the 3 x 3 sharpening filter, reflect-101.
// Everything is integer work except CLAHE's table scale and blend, whose float32 form is augment_ext_u8.hip's (every operation
// rounded on its own: contraction is off for this file), and the boost, one float32 product.  Results equal tests/textenh_ref.py
// byte for byte and do not depend on the schedule.
//
// Eleven launches, whatever the images hold: prep (one workgroup: validates the descriptors, lays the images' planes out one after
// the other) -> grey -> tile tables -> blend -> Sobel magnitude -> suppression + labels -> joins -> roots + strong flags -> edges -> dilate
// -> boost + sharpen.  Every per-pixel launch is a (ceil(max_pixels / 256), N) grid; workgroups past their image leave at once.
//
// Hysteresis: the edge image is 255 on the candidates (magnitude above the low threshold that survive the suppression) that are
// 8-connected, through candidates, to one above the high threshold.  That is a component property, so it is computed with one
// union-find pass in the scheme of mask_post.hip: a label holds parent + 1 (0 = no candidate), a parent is never greater than its
// child, every find / union chain strictly descends and ends by its own progress; the joins, the marking of the roots that hold a
// strong pixel (integer atomicMax on a flag per root) and the read-out are separate launches.  No wait on another workgroup.
#include "uwm_kernels.h"

namespace uwm {

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

#include "image_common.inc"

constexpr int kThreads = 256;
constexpr int kMinSide = 16;                 // an image with a shorter side is copied through (status 2)
constexpr int kLow = 50, kHigh = 150;        // Canny's thresholds on |dx| + |dy|
constexpr int kTg22 = 13573;                 // tan(22.5 deg) in 15 fraction bits, cv2's TG22

struct Rec {                   // one per image, written by te_prep.  mode 0: misfit, 1: enhanced, 2: copied through
  long long off, eoff, pix;    // bytes into in / out, bytes into edges, pixels into the planes of the workspace
  int h, w, mode;
  int th, tw, clip;            // CLAHE: the tile of the padded image, the integer clip limit
  float inv_th, inv_tw, scale; // 1.0f / th, 1.0f / tw, 255.0f / (th * tw)
};

// ---------------------------------------------------------------- prep
// One workgroup: validates every descriptor and gives each enhanced image its place in the planes (prefix sums over N in turns of
// kThreads images).  Misfit: a side outside 1 .. 2^30, h * w > max_pixels, a region that leaves in / out or edges, an edge
// descriptor of another size, or planes that would pass total_pixels.
__global__ void __launch_bounds__(kThreads) te_prep(const ImageDesc* __restrict__ descs, const ImageDesc* __restrict__ edescs, Rec* __restrict__ recs,
                                                    int* __restrict__ status, int N, long long bytes, long long edges_bytes, long long max_pixels,
                                                    long long total_pixels) {
  __shared__ long long s_pix[kThreads], s_carry;
  const int t = threadIdx.x;
  if (t == 0) s_carry = 0;
  for (int base = 0; base < N; base += kThreads) {
    __syncthreads();
    const int i = base + t;
    Rec r = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1.0f, 1.0f, 1.0f};
    long long area = 0;
    if (i < N) {
      const ImageDesc d = descs[i];
      bool ok = region_ok(d, 3, (size_t)bytes);
      area = ok ? (long long)d.h * d.w : 0;
      ok = ok && area <= max_pixels;
      if (ok && edescs) {
        const ImageDesc e = edescs[i];
        ok = e.h == d.h && e.w == d.w && region_ok(e, 1, (size_t)edges_bytes);
        r.eoff = ok ? e.offset : 0;
      }
      if (ok) { r.off = d.offset; r.h = d.h; r.w = d.w; r.mode = (d.h >= kMinSide && d.w >= kMinSide) ? 1 : 2; }
    }
    const long long mine = r.mode == 1 ? area : 0;
    s_pix[t] = mine;
    block_scan_incl(s_pix, t);
    const long long to = s_carry + s_pix[t];
    if (r.mode == 1) {
      if (to > total_pixels) { r = Rec{0, 0, 0, 0, 0, 0, 1, 1, 1, 1.0f, 1.0f, 1.0f}; }
      else {
        r.pix = to - mine;
        // cv2's CLAHE: the image is padded only when a side is no multiple of 8, and then BOTH sides grow, by 8 - side % 8
        const bool pad = (r.h & 7) || (r.w & 7);
        const int hp = pad ? r.h + 8 - (r.h & 7) : r.h, wp = pad ? r.w + 8 - (r.w & 7) : r.w;
        r.th = hp >> 3; r.tw = wp >> 3;
        const long long ta = (long long)r.th * r.tw;
        r.clip = (int)max((2 * ta) >> 8, 1ll);                // max(int(2.0 * th * tw / 256), 1)
        r.inv_th = 1.0f / (float)r.th;
        r.inv_tw = 1.0f / (float)r.tw;
        r.scale = 255.0f / (float)ta;
      }
    }
    if (i < N) { recs[i] = r; status[i] = r.mode == 1 ? 0 : r.mode == 2 ? 2 : 1; }
    __syncthreads();
    if (t == kThreads - 1) s_carry = to;
  }
}

// ---------------------------------------------------------------- grey (mode 2: the copy through)
__global__ void __launch_bounds__(kThreads) te_grey(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint8_t* __restrict__ edges,
                                                    const Rec* __restrict__ recs, uint8_t* __restrict__ grey) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode == 0) return;
  const long long total = (long long)rc.h * rc.w, p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= total) return;
  const uint8_t* px = in + rc.off + 3 * p;
  const int r = px[0], g = px[1], b = px[2];
  if (rc.mode == 2) {
    uint8_t* o = out + rc.off + 3 * p;
    o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
    if (edges) edges[rc.eoff + p] = 0;
    return;
  }
  grey[rc.pix + p] = (uint8_t)((r * 9798 + g * 19235 + b * 3735 + 16384) >> 15);
}

// ---------------------------------------------------------------- CLAHE
// One workgroup = one tile of one image: 256-bin histogram of the padded tile (reflect-101) in LDS, clip, redistribute, prefix sum,
// table -> luts [N][64][256].  The arithmetic is augment_ext_hist_kernel's.
__global__ void __launch_bounds__(256) te_hist(const uint8_t* __restrict__ grey, const Rec* __restrict__ recs, uint8_t* __restrict__ luts) {
  const int n = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  const Rec rc = recs[n];
  if (rc.mode != 1) return;                                  // uniform, before any barrier
  __shared__ int hist[256];
  __shared__ int scan[2][256];
  __shared__ int s_excess;
  hist[t] = 0;
  if (t == 0) s_excess = 0;
  __syncthreads();
  const uint8_t* __restrict__ img = grey + rc.pix;
  const int H = rc.h, W = rc.w, th = rc.th, tw = rc.tw;
  const int y0 = (tile >> 3) * th, x0 = (tile & 7) * tw, area = th * tw;
  for (int i = t; i < area; i += 256) {
    const int dy = i / tw, dx = i - dy * tw;
    atomicAdd(&hist[img[(size_t)reflect101_near(y0 + dy, H) * W + reflect101_near(x0 + dx, W)]], 1);
  }
  __syncthreads();
  const int clip = rc.clip;
  int h = hist[t];
  if (h > clip) atomicAdd(&s_excess, h - clip);
  __syncthreads();
  const int excess = s_excess, batch = excess >> 8, resid = excess - (batch << 8);
  h = min(h, clip) + batch;
  if (resid) {
    const int step = max(256 / resid, 1);
    if (t % step == 0 && t / step < resid) ++h;
  }
  scan[0][t] = h;
  __syncthreads();
  int cur = 0;
#pragma unroll
  for (int d = 1; d < 256; d <<= 1) {
    scan[cur ^ 1][t] = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  luts[((size_t)n * 64 + tile) * 256 + t] = (uint8_t)clamp255(__float2int_rn((float)scan[cur][t] * rc.scale));
}

__global__ void __launch_bounds__(kThreads) te_clahe(const uint8_t* __restrict__ grey, const Rec* __restrict__ recs, const uint8_t* __restrict__ luts,
                                                     uint8_t* __restrict__ cl) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode != 1) return;
  const long long total = (long long)rc.h * rc.w, p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= total) return;
  const int y = (int)((unsigned)p / (unsigned)rc.w), x = (int)p - y * rc.w;      // (p < 2^30: 32-bit division)
  const int l = grey[rc.pix + p];
  const uint8_t* __restrict__ lut = luts + (size_t)blockIdx.y * 64 * 256;
  int ty1, ty2, tx1, tx2;
  float ya, xa;
  clahe_axis(y, rc.inv_th, ty1, ty2, ya);
  clahe_axis(x, rc.inv_tw, tx1, tx2, xa);
  const float ya1 = 1.0f - ya, xa1 = 1.0f - xa;
  const float l11 = lut[(ty1 * 8 + tx1) * 256 + l], l12 = lut[(ty1 * 8 + tx2) * 256 + l];
  const float l21 = lut[(ty2 * 8 + tx1) * 256 + l], l22 = lut[(ty2 * 8 + tx2) * 256 + l];
  const float top = l11 * xa1 + l12 * xa, bot = l21 * xa1 + l22 * xa;
  cl[rc.pix + p] = (uint8_t)clamp255(__float2int_rn(top * ya1 + bot * ya));
}

// ---------------------------------------------------------------- Canny
// the 3 x 3 Sobel derivatives at (y, x), BORDER_REPLICATE
__device__ __forceinline__ void sobel(const uint8_t* __restrict__ img, int H, int W, int y, int x, int& dx, int& dy) {
  const int ym = max(y - 1, 0), yp = min(y + 1, H - 1), xm = max(x - 1, 0), xp = min(x + 1, W - 1);
  const uint8_t* r0 = img + (size_t)ym * W;
  const uint8_t* r1 = img + (size_t)y * W;
  const uint8_t* r2 = img + (size_t)yp * W;
  const int a = r0[xm], b = r0[x], c = r0[xp], d = r1[xm], f = r1[xp], g = r2[xm], h = r2[x], k = r2[xp];
  dx = (c + 2 * f + k) - (a + 2 * d + g);
  dy = (g + 2 * h + k) - (a + 2 * b + c);
}

__global__ void __launch_bounds__(kThreads) te_sobel(const uint8_t* __restrict__ cl, const Rec* __restrict__ recs, unsigned short* __restrict__ mag) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode != 1) return;
  const long long total = (long long)rc.h * rc.w, p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= total) return;
  const int y = (int)((unsigned)p / (unsigned)rc.w), x = (int)p - y * rc.w;      // (p < 2^30: 32-bit division)
  int dx, dy;
  sobel(cl + rc.pix, rc.h, rc.w, y, x, dx, dy);
  mag[rc.pix + p] = (unsigned short)(abs(dx) + abs(dy));       // at most 2040
}

// Non-maximum suppression -> labels: 0, or for a candidate the start of its run inside the wave's 64 pixels (+ 1); flags = 0.
// Magnitude outside the image is 0.  Every lane of a wave reaches the ballots (workgroups wholly past the image have left).
__global__ void __launch_bounds__(kThreads) te_nms(const uint8_t* __restrict__ cl, const unsigned short* __restrict__ mag, const Rec* __restrict__ recs,
                                                   int* __restrict__ labels, int* __restrict__ flags) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode != 1) return;
  const int H = rc.h, W = rc.w;
  const long long total = (long long)H * W;
  if ((long long)blockIdx.x * kThreads >= total) return;       // uniform in the workgroup
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool inside = p < total;
  bool cand = false;
  int x = 1;
  if (inside) {
    const int y = (int)((unsigned)p / (unsigned)W);            // (p < 2^30: 32-bit division)
    x = (int)p - y * W;
    const unsigned short* __restrict__ mg = mag + rc.pix;
    const int m = mg[p];
    if (m > kLow) {
      int xs, ys;
      sobel(cl + rc.pix, H, W, y, x, xs, ys);
      const int ax = abs(xs), ay = abs(ys) << 15, tg22 = ax * kTg22;
      if (ay < tg22) {                                         // horizontal gradient
        const int l = x > 0 ? mg[p - 1] : 0, r = x + 1 < W ? mg[p + 1] : 0;
        cand = m > l && m >= r;
      } else if (ay > tg22 + (ax << 16)) {                     // vertical gradient
        const int u = y > 0 ? mg[p - W] : 0, d = y + 1 < H ? mg[p + W] : 0;
        cand = m > u && m >= d;
      } else {                                                 // diagonal
        const int s = (xs ^ ys) < 0 ? -1 : 1;
        const int xu = x - s, xd = x + s;
        const int u = (y > 0 && xu >= 0 && xu < W) ? mg[p - W - s] : 0;
        const int d = (y + 1 < H && xd >= 0 && xd < W) ? mg[p + W + s] : 0;
        cand = m > u && m > d;
      }
    }
  }
  const int lane = threadIdx.x & 63;
  const u64 bits = __ballot(cand), rowstart = __ballot(x == 0);
  if (!inside) return;
  int l = 0;
  if (cand) {
    // a run starts at lane 0, behind a lane that is no candidate, and at the first pixel of a row
    const u64 starts = ((~bits << 1) | rowstart | 1ull) & ((2ull << lane) - 1ull);
    const int start = 63 - __clzll((long long)starts);
    l = (int)p - lane + start + 1;
  }
  labels[rc.pix + p] = l;
  flags[rc.pix + p] = 0;
}

// joins across the 64-pixel groups and between rows (cc_join, 8-connected; the set is the candidates: label != 0)
__global__ void __launch_bounds__(kThreads) te_merge(const Rec* __restrict__ recs, int* __restrict__ labels) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode != 1) return;
  const int H = rc.h, W = rc.w;
  const long long total = (long long)H * W, pl = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (pl >= total) return;
  const int p = (int)pl, y = p / W, x = p - y * W;
  int* lab = labels + rc.pix;
  if (ld_label(lab + p) == 0) return;
  cc_join<true, 1>(lab, p, x, y, W, [&](int dy, int dx) { return ld_label(lab + p + dy * W + dx) != 0; }, (p & 63) == 0);
}

// labels <- root + 1 (a root is an ancestor of everything a walk meets on its way, so the stores of other threads only shorten
// it), and the root of every candidate above the high threshold gets its flag
__global__ void __launch_bounds__(kThreads) te_strong(const unsigned short* __restrict__ mag, const Rec* __restrict__ recs,
                                                      int* __restrict__ labels, int* __restrict__ flags) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode != 1) return;
  const long long total = (long long)rc.h * rc.w, p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= total) return;
  int* lab = labels + rc.pix;
  if (ld_label(lab + p) == 0) return;
  const int r = uf_find<1>(lab, (int)p);
  st_label(lab + p, r + 1);
  if (mag[rc.pix + p] > kHigh) atomicMax(flags + rc.pix + r, 1);
}

__global__ void __launch_bounds__(kThreads) te_edges(const Rec* __restrict__ recs, const int* __restrict__ labels, const int* __restrict__ flags,
                                                     uint8_t* __restrict__ edge) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode != 1) return;
  const long long total = (long long)rc.h * rc.w, p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= total) return;
  const int l = labels[rc.pix + p];                            // root + 1 since te_strong
  edge[rc.pix + p] = (l != 0 && flags[rc.pix + l - 1] != 0) ? 255 : 0;
}

// ---------------------------------------------------------------- dilate, boost, sharpen
// getStructuringElement(MORPH_ELLIPSE, (2, 2)) = [[0, 1], [1, 1]], anchor (1, 1): the pixel, the one above, the one to the left
__global__ void __launch_bounds__(kThreads) te_dilate(const Rec* __restrict__ recs, const uint8_t* __restrict__ edge, uint8_t* __restrict__ dil,
                                                      uint8_t* __restrict__ edges_out) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode != 1) return;
  const long long total = (long long)rc.h * rc.w, p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= total) return;
  const int y = (int)((unsigned)p / (unsigned)rc.w), x = (int)p - y * rc.w;      // (p < 2^30: 32-bit division)
  const uint8_t* e = edge + rc.pix;
  int v = e[p];
  if (y > 0) v |= e[p - rc.w];
  if (x > 0) v |= e[p - 1];
  dil[rc.pix + p] = (uint8_t)v;
  if (edges_out) edges_out[rc.eoff + p] = (uint8_t)v;
}

__device__ __forceinline__ int boost(int v) { return (int)fminf((float)v * 1.2f, 255.0f); }      // one float32 product, truncated

// out = clamp(9 c - the 8 neighbours) of the boosted image = clamp(10 c - the 9 taps), BORDER_REFLECT_101 (sides >= 16)
__global__ void __launch_bounds__(kThreads) te_final(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Rec* __restrict__ recs,
                                                     const uint8_t* __restrict__ dil) {
  const Rec rc = recs[blockIdx.y];
  if (rc.mode != 1) return;
  const int H = rc.h, W = rc.w;
  const long long total = (long long)H * W, p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= total) return;
  const int y = (int)((unsigned)p / (unsigned)W), x = (int)p - y * W;          // (p < 2^30: 32-bit division)
  const uint8_t* __restrict__ img = in + rc.off;
  const uint8_t* __restrict__ d = dil + rc.pix;
  int sum[3] = {0, 0, 0}, ctr[3] = {0, 0, 0};
#pragma unroll
  for (int j = -1; j <= 1; ++j) {
    const int yy = reflect101_near(y + j, H);
#pragma unroll
    for (int i = -1; i <= 1; ++i) {
      const int xx = reflect101_near(x + i, W);
      const size_t q = (size_t)yy * W + xx;
      const bool e = d[q] != 0;
      const uint8_t* px = img + 3 * q;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int v = e ? boost(px[c]) : px[c];
        sum[c] += v;
        if (i == 0 && j == 0) ctr[c] = v;
      }
    }
  }
  uint8_t* o = out + rc.off + 3 * p;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (uint8_t)clamp255(10 * ctr[c] - sum[c]);
}

// ---------------------------------------------------------------- host side
struct Layout {                // workspace: status, records, tables, grey / edge plane, CLAHE / dilated plane, magnitudes, labels, flags
  size_t recs, luts, grey, cl, mag, labels, flags, total;
};
Layout layout(int N, long long total_pixels) {
  Layout l;
  const size_t tp = (size_t)total_pixels;
  l.recs = rup256((size_t)N * sizeof(int));
  l.luts = l.recs + rup256((size_t)N * sizeof(Rec));
  l.grey = l.luts + rup256((size_t)N * 64 * 256);
  l.cl = l.grey + rup256(tp);
  l.mag = l.cl + rup256(tp);
  l.labels = l.mag + rup256(tp * 2);
  l.flags = l.labels + rup256(tp * 4);
  l.total = l.flags + rup256(tp * 4);
  return l;
}

}  // namespace

size_t text_enhance_workspace_bytes(long long total_pixels, int N) { return layout(N, total_pixels).total; }

hipError_t launch_text_enhance_ragged(const uint8_t* in, uint8_t* out, size_t bytes, const ImageDesc* descs, int N, long long max_pixels,
                                      long long total_pixels, uint8_t* edges, size_t edges_bytes, const ImageDesc* edge_descs, void* ws,
                                      hipStream_t st) {
  const Layout l = layout(N, total_pixels);
  char* w = (char*)ws;
  int* status = (int*)w;
  Rec* recs = (Rec*)(w + l.recs);
  uint8_t* luts = (uint8_t*)(w + l.luts);
  uint8_t* grey = (uint8_t*)(w + l.grey);                      // later the edge plane
  uint8_t* cl = (uint8_t*)(w + l.cl);                          // later the dilated plane
  unsigned short* mag = (unsigned short*)(w + l.mag);
  int* labels = (int*)(w + l.labels);
  int* flags = (int*)(w + l.flags);
  const dim3 grid((unsigned)((max_pixels + kThreads - 1) / kThreads), (unsigned)N), block(kThreads);
  hipLaunchKernelGGL(te_prep, dim3(1), block, 0, st, descs, edges ? edge_descs : nullptr, recs, status, N, (long long)bytes,
                     (long long)edges_bytes, max_pixels, total_pixels);
  hipLaunchKernelGGL(te_grey, grid, block, 0, st, in, out, edges, recs, grey);
  hipLaunchKernelGGL(te_hist, dim3(64, (unsigned)N), dim3(256), 0, st, grey, recs, luts);
  hipLaunchKernelGGL(te_clahe, grid, block, 0, st, grey, recs, luts, cl);
  hipLaunchKernelGGL(te_sobel, grid, block, 0, st, cl, recs, mag);
  hipLaunchKernelGGL(te_nms, grid, block, 0, st, cl, mag, recs, labels, flags);
  hipLaunchKernelGGL(te_merge, grid, block, 0, st, recs, labels);
  hipLaunchKernelGGL(te_strong, grid, block, 0, st, mag, recs, labels, flags);
  hipLaunchKernelGGL(te_edges, grid, block, 0, st, recs, labels, flags, grey);
  hipLaunchKernelGGL(te_dilate, grid, block, 0, st, recs, grey, cl, edges);
  hipLaunchKernelGGL(te_final, grid, block, 0, st, in, out, recs, cl);
  return hipGetLastError();
}

}  // namespace uwm
