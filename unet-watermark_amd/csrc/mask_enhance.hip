// Mask enhancement on the device: the reference's enhance_mask (src/scripts/enhance_masks.py) for a ragged batch of 8-bit grey
// masks.  DESIGN.md §8l is the specification.  The chain that runs is the reduced one (the two reductions are exact and the CPU
// tests hold them):
//   grey close E(7,7)  ->  grey dilate E(2e+1, 2e+1)  ->  float Gaussian blur, reflect-101  ->  > 127  ->  s x (open E(5,5), close E(5,5))
// Every stage (two smoothing rounds count as one) is one launch over (tiles, images); a stage reads a plane and writes another, so
// `out` may be `in`: the input is read by the first stage only, the output is written by the last stage only, everything between
// lives in the two planes of the workspace, which use the masks' own offsets.  Results are exact: integer min / max, and a blur whose every float operation is
// fixed (below), so they do not depend on the schedule.
//
// Morphology (me_morph): a workgroup takes a 64 x 64 tile with a halo of the element's radius r into LDS.  An element row is a
// horizontal span of 2*dx + 1, so the result is the max (min) over the rows of a horizontal windowed max (min).  The widths
// differ from row to row, so the tile's rows are turned level by level into a doubling table, L_k[x] = max of the 2^k pixels
// from x on, and a span of width v with 2^k <= v < 2^(k+1) is max(L_k[x - dx], L_k[x + dx + 1 - 2^k]): two reads, whatever v is.
// Only two levels are alive at a time (ping-pong): each thread keeps its 16 results in registers and serves, at level k, the rows
// whose width falls into that level.  LDS: 2 x 126 x 128 bytes.  Outside the image: 0 for max, 255 for min (ignored).
//
// The binary smoothing rounds do not go through me_morph: me_smooth (below) runs two rounds, eight passes, in LDS per launch.
//
// Blur + threshold (me_blur): the same tile with a halo of the Gaussian's radius, fetched through reflect-101 (of any
// coordinate, so images narrower than the radius work); the row pass goes to a float32 LDS plane, the column pass reads
// it and thresholds.  Each pass is acc = t[c] * x[0]; acc += t[c + i] * (x[-i] + x[+i]) for i = 1 .. r in order, every operation
// rounded to float32 (__fmul_rn / __fadd_rn: no contraction).  blur_kernel 0 is the one-tap kernel {1}: x * 1 is x.
#include "uwm_kernels.h"

#include <cmath>

namespace uwm {

namespace {

#include "image_common.inc"

constexpr int kThreads = 256;
constexpr int kT = 64;                         // tile side
constexpr int kMaxR = 31;                      // largest radius: ellipse 63, Gaussian 63
constexpr int kSide = kT + 2 * kMaxR;          // 126: tile + halo
constexpr int kPer = kT * kT / kThreads;       // results per thread: rows (tid >> 6) + 4 j, column tid & 63

struct Rec {                   // one per image, written by me_prep; h == 0: misfit
  long long off;
  int h, w;
};
struct Ellipse {               // cv2's MORPH_ELLIPSE of side 2r + 1: row i spans [r - dx[i], r + dx[i]]
  int r;
  unsigned char dx[2 * kMaxR + 1];
};
struct Taps {                  // the upper half of the symmetric kernel: t[i] = tap c + i
  int r;
  float t[kMaxR + 1];
};

// validates descriptor i (the rule of uwm_optimize_masks_ragged, without its row capacity) and fills stats[i] = {0, 0, h*w, 0} or
// {0, 0, 0, 1}; the counts are added by me_count
__global__ void __launch_bounds__(kThreads) me_prep(const ImageDesc* __restrict__ descs, Rec* __restrict__ recs, long long* __restrict__ stats,
                                                    int N, long long mask_bytes, long long max_pixels) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const ImageDesc d = descs[i];
  Rec r = {0, 0, 0};
  const long long area = (long long)d.h * d.w;                  // (read only where region_ok holds)
  if (region_ok(d, 1, (size_t)mask_bytes) && area <= max_pixels) { r.off = d.offset; r.h = d.h; r.w = d.w; }
  recs[i] = r;
  if (stats) {
    long long* s = stats + (size_t)i * 4;
    s[0] = 0; s[1] = 0;
    s[2] = r.h ? area : 0;
    s[3] = r.h ? 0 : 1;
  }
}

// stats[n][slot] += pixels > 127 of image n in buf (integer sums: the same on every run)
__global__ void __launch_bounds__(kThreads) me_count(const uint8_t* __restrict__ buf, const Rec* __restrict__ recs, long long* __restrict__ stats,
                                                     int slot) {
  __shared__ unsigned s_cnt[kThreads / 64];
  const Rec rc = recs[blockIdx.y];
  if (rc.h == 0) return;
  const long long total = (long long)rc.h * rc.w;
  if ((long long)blockIdx.x * kThreads >= total) return;
  const uint8_t* img = buf + rc.off;
  unsigned cnt = 0;
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < total; p += (long long)gridDim.x * kThreads) cnt += img[p] > 127;
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
    for (int k = 0; k < kThreads / 64; ++k) sum += s_cnt[k];
    if (sum) atomicAdd((unsigned long long*)(stats + (size_t)blockIdx.y * 4 + slot), sum);
  }
}

template <bool MAX>
__device__ __forceinline__ int mm(int a, int b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); }

// n / d by a multiplication: exact for the tile indices here (n < 2^14, d <= 128 and n / d < 2^7: n * (m*d - 2^24) < 2^24, n * m < 2^32)
struct Div {
  unsigned m;
  __device__ __forceinline__ explicit Div(int d) : m(((1u << 24) + d - 1) / d) {}
  __device__ __forceinline__ int operator()(int n) const { return (int)(((unsigned)n * m) >> 24); }
};
constexpr int kFetch = 8;                      // global loads a thread keeps in flight while a tile is fetched
constexpr int kPitch = (kSide + 3) & ~3;       // 128: the widest LDS row of byte cells, a whole number of dwords

// A tile is fetched four cells to a lane: cells gx .. gx + 3 of image row gy as a dword, cell k in byte k.  Where the four lie
// inside the row this is ONE load of four bytes at the cells' own alignment; a byte load per lane keeps too few bytes in flight
// to reach the memory's rate.  A cell outside the image reads `outside`.  No load touches a byte outside the image.
__device__ __forceinline__ unsigned fetch4(const uint8_t* __restrict__ img, int H, int W, int gy, int gx, unsigned outside) {
  if (gy < 0 || gy >= H) return outside * 0x01010101u;
  const size_t row = (size_t)gy * W;
  if (gx >= 0 && gx + 3 < W) {
    unsigned v;
    __builtin_memcpy(&v, img + row + gx, 4);
    return v;
  }
  unsigned v = 0;
  for (int k = 0; k < 4; ++k) {
    const int x = gx + k;
    v |= (x >= 0 && x < W ? (unsigned)img[row + x] : outside) << (8 * k);
  }
  return v;
}
// the same through BORDER_REFLECT_101
__device__ __forceinline__ unsigned fetch4_reflect(const uint8_t* __restrict__ img, int H, int W, int gy, int gx) {
  const size_t row = (size_t)reflect101(gy, H) * W;
  if (gx >= 0 && gx + 3 < W) {
    unsigned v;
    __builtin_memcpy(&v, img + row + gx, 4);
    return v;
  }
  unsigned v = 0;
  for (int k = 0; k < 4; ++k) v |= (unsigned)img[row + reflect101(gx + k, W)] << (8 * k);
  return v;
}

template <bool MAX>
__global__ void __launch_bounds__(kThreads) me_morph(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const Rec* __restrict__ recs,
                                                     Ellipse el) {
  __shared__ unsigned s_a[kSide * kPitch / 4], s_b[kSide * kPitch / 4];
  const Rec rc = recs[blockIdx.y];
  if (rc.h == 0) return;
  const int H = rc.h, W = rc.w, r = el.r;
  const uint8_t* img = src + rc.off;
  uint8_t* out = dst + rc.off;
  const int outside = MAX ? 0 : 255;
  const int top = 31 - __clz(2 * r + 1);                   // the level of the widest row
  const int ntx = (W + kT - 1) / kT;
  const long long ntiles = (long long)ntx * ((H + kT - 1) / kT);
  const int tid = threadIdx.x, lx = tid & 63, ly0 = tid >> 6;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {       // (uniform in the workgroup)
    const int y0 = (int)(t / ntx) * kT, x0 = (int)(t % ntx) * kT;
    const int th = H - y0 < kT ? H - y0 : kT, tw = W - x0 < kT ? W - x0 : kT;
    const int PH = th + 2 * r, PQ = (tw + 2 * r + 3) / 4, PW = 4 * PQ, quads = PH * PQ, cells = PH * PW;      // rows of PQ dwords
    const Div by_pq(PQ), by_pw(PW);
    __syncthreads();                                       // the previous tile's reads are over
    for (int base = tid; base < quads; base += kFetch * kThreads) {
      unsigned v[kFetch];
#pragma unroll
      for (int u = 0; u < kFetch; ++u) {
        const int idx = base + u * kThreads, ty = by_pq(idx);
        v[u] = idx < quads ? fetch4(img, H, W, y0 - r + ty, x0 - r + 4 * (idx - ty * PQ), outside) : 0u;
      }
#pragma unroll
      for (int u = 0; u < kFetch; ++u)
        if (base + u * kThreads < quads) s_a[base + u * kThreads] = v[u];
    }
    __syncthreads();
    int acc[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) acc[j] = outside;
    uint8_t* cur = (uint8_t*)s_a;
    uint8_t* nxt = (uint8_t*)s_b;
    for (int k = 0;; ++k) {
      const int span = 1 << k;                             // cur[x] = max / min of the `span` pixels from x on
      for (int i = 0; i <= 2 * r; ++i) {
        const int dx = el.dx[i];
        if (31 - __clz(2 * dx + 1) != k) continue;
        const int c0 = i * PW + r - dx, c1 = i * PW + r + dx + 1 - span;
        if (lx < tw) {
#pragma unroll
          for (int j = 0; j < kPer; ++j) {
            const int ly = ly0 + 4 * j;
            if (ly < th) {
              const uint8_t* p = cur + ly * PW + lx;
              acc[j] = mm<MAX>(acc[j], mm<MAX>(p[c0], p[c1]));
            }
          }
        }
      }
      if (k == top) break;
      for (int idx = tid; idx < cells; idx += kThreads) {
        const int tx = idx - by_pw(idx) * PW, a = cur[idx];
        nxt[idx] = (uint8_t)(tx + span < PW ? mm<MAX>(a, cur[idx + span]) : a);     // (a window that leaves the row is never asked for)
      }
      __syncthreads();
      uint8_t* sw = cur; cur = nxt; nxt = sw;
    }
    if (lx < tw) {
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int ly = ly0 + 4 * j;
        if (ly < th) out[(size_t)(y0 + ly) * W + x0 + lx] = (uint8_t)acc[j];
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) me_blur(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const Rec* __restrict__ recs,
                                                    Taps tp) {
  __shared__ unsigned s_q[kSide * kPitch / 4];
  __shared__ float s_row[kSide * kT];
  const Rec rc = recs[blockIdx.y];
  if (rc.h == 0) return;
  const int H = rc.h, W = rc.w, r = tp.r;
  const uint8_t* img = src + rc.off;
  uint8_t* out = dst + rc.off;
  const int ntx = (W + kT - 1) / kT;
  const long long ntiles = (long long)ntx * ((H + kT - 1) / kT);
  const int tid = threadIdx.x, lx = tid & 63, ly0 = tid >> 6;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {       // (uniform in the workgroup)
    const int y0 = (int)(t / ntx) * kT, x0 = (int)(t % ntx) * kT;
    const int th = H - y0 < kT ? H - y0 : kT, tw = W - x0 < kT ? W - x0 : kT;
    const int PH = th + 2 * r, PQ = (tw + 2 * r + 3) / 4, PW = 4 * PQ, quads = PH * PQ;       // rows of PQ dwords
    const Div by_pq(PQ), by_tw(tw);
    const uint8_t* s_in = (const uint8_t*)s_q;
    __syncthreads();                                       // the previous tile's reads are over
    for (int base = tid; base < quads; base += kFetch * kThreads) {
      unsigned v[kFetch];
#pragma unroll
      for (int u = 0; u < kFetch; ++u) {
        const int idx = base + u * kThreads, ty = by_pq(idx);
        v[u] = idx < quads ? fetch4_reflect(img, H, W, y0 - r + ty, x0 - r + 4 * (idx - ty * PQ)) : 0u;
      }
#pragma unroll
      for (int u = 0; u < kFetch; ++u)
        if (base + u * kThreads < quads) s_q[base + u * kThreads] = v[u];
    }
    __syncthreads();
    for (int idx = tid; idx < PH * tw; idx += kThreads) {  // rows, halo rows included
      const int ty = by_tw(idx), x = idx - ty * tw;
      const uint8_t* p = s_in + ty * PW + x + r;
      float acc = __fmul_rn(tp.t[0], (float)p[0]);
      for (int i = 1; i <= r; ++i) acc = __fadd_rn(acc, __fmul_rn(tp.t[i], __fadd_rn((float)p[-i], (float)p[i])));
      s_row[ty * kT + x] = acc;
    }
    __syncthreads();
    if (lx < tw) {
#pragma unroll 4
      for (int j = 0; j < kPer; ++j) {
        const int ly = ly0 + 4 * j;
        if (ly < th) {
          const float* q = s_row + (ly + r) * kT + lx;
          float acc = __fmul_rn(tp.t[0], q[0]);
          for (int i = 1; i <= r; ++i) acc = __fadd_rn(acc, __fmul_rn(tp.t[i], __fadd_rn(q[-i * kT], q[i * kT])));
          out[(size_t)(y0 + ly) * W + x0 + lx] = acc > 127.0f ? 255 : 0;
        }
      }
    }
  }
}

// Binary smoothing: `rounds` (1 .. kSR) rounds of open, close E(5,5) = erode, dilate, dilate, erode on a {0,255} plane, all in LDS.
// A pass reaches 2 pixels, so the tile carries a halo of 8 per round and whatever the unknown cells beyond the halo spoil stops
// short of the tile.  Cells are bytes, four to a dword: on {0,255} max is OR and min is AND, and a pass is, per dword, the
// horizontal 5-span h (two neighbour dwords, byte-aligned shifts) and then h[y-1] . h[y] . h[y+1] . a[y-2] . a[y+2] — E(5,5) is rows of
// 1, 5, 5, 5, 1.  Cells outside the image are rewritten after every pass with what the NEXT pass ignores (255 for an erosion).
constexpr int kSR = 2;                         // rounds per launch
constexpr int kSS = kT + 2 * 8 * kSR;          // 96: tile + halo
constexpr int kSP = kSS / 4;                   // dwords per row

__device__ __forceinline__ unsigned shr_bytes(unsigned hi, unsigned lo, int n) {          // bytes n .. n + 3 of hi:lo
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * n));
}

__global__ void __launch_bounds__(kThreads) me_smooth(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const Rec* __restrict__ recs,
                                                      int rounds) {
  __shared__ unsigned s_a[kSS * kSP], s_b[kSS * kSP], s_h[kSS * kSP], s_col[kSP];
  const Rec rc = recs[blockIdx.y];
  if (rc.h == 0) return;
  const int H = rc.h, W = rc.w, halo = 8 * rounds;
  const uint8_t* img = src + rc.off;
  uint8_t* out = dst + rc.off;
  const int ntx = (W + kT - 1) / kT;
  const long long ntiles = (long long)ntx * ((H + kT - 1) / kT);
  const int tid = threadIdx.x, lx = tid & 63, ly0 = tid >> 6;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {       // (uniform in the workgroup)
    const int y0 = (int)(t / ntx) * kT, x0 = (int)(t % ntx) * kT;
    const int th = H - y0 < kT ? H - y0 : kT, tw = W - x0 < kT ? W - x0 : kT;
    const int PH = th + 2 * halo, PD = (tw + 2 * halo + 3) / 4, words = PH * PD;
    const Div by_pd(PD);
    __syncthreads();                                       // the previous tile's reads are over
    if (tid < PD) {                                        // which bytes of a row's dword tid lie inside the image
      unsigned m = 0;
      for (int k = 0; k < 4; ++k) {
        const int gx = x0 - halo + 4 * tid + k;
        if (gx >= 0 && gx < W) m |= 0xffu << (8 * k);
      }
      s_col[tid] = m;
    }
    for (int base = tid; base < words; base += kFetch * kThreads) {
      unsigned v[kFetch];
#pragma unroll
      for (int u = 0; u < kFetch; ++u) {
        const int idx = base + u * kThreads, ty = by_pd(idx);
        v[u] = idx < words ? fetch4(img, H, W, y0 - halo + ty, x0 - halo + 4 * (idx - ty * PD), 255u) : 0u;     // the first pass is an erosion
      }
#pragma unroll
      for (int u = 0; u < kFetch; ++u) {
        const int idx = base + u * kThreads, ty = by_pd(idx);
        if (idx < words) s_a[ty * kSP + idx - ty * PD] = v[u];
      }
    }
    __syncthreads();
    unsigned* a = s_a;
    unsigned* b = s_b;
    for (int p = 0; p < 4 * rounds; ++p) {
      const bool is_or = (p & 3) == 1 || (p & 3) == 2, next_or = ((p + 1) & 3) == 1 || ((p + 1) & 3) == 2;
      for (int idx = tid; idx < words; idx += kThreads) {
        const int y = by_pd(idx), j = idx - y * PD;
        const unsigned* row = a + y * kSP;
        const unsigned c = row[j], l = j > 0 ? row[j - 1] : c, n = j + 1 < PD ? row[j + 1] : c;
        const unsigned x1 = shr_bytes(n, c, 1), x2 = shr_bytes(n, c, 2), x3 = shr_bytes(c, l, 3), x4 = shr_bytes(c, l, 2);
        s_h[y * kSP + j] = is_or ? (c | x1 | x2 | x3 | x4) : (c & x1 & x2 & x3 & x4);
      }
      __syncthreads();
      for (int idx = tid; idx < words; idx += kThreads) {
        const int y = by_pd(idx), j = idx - y * PD;
        const int u1 = y > 0 ? y - 1 : 0, u2 = y > 1 ? y - 2 : 0, d1 = y + 1 < PH ? y + 1 : PH - 1, d2 = y + 2 < PH ? y + 2 : PH - 1;
        const unsigned h0 = s_h[y * kSP + j], h1 = s_h[u1 * kSP + j], h2 = s_h[d1 * kSP + j], a1 = a[u2 * kSP + j], a2 = a[d2 * kSP + j];
        const unsigned v = is_or ? (h0 | h1 | h2 | a1 | a2) : (h0 & h1 & h2 & a1 & a2);
        const int gy = y0 - halo + y;
        const unsigned m = gy >= 0 && gy < H ? s_col[j] : 0u;
        b[y * kSP + j] = (v & m) | (next_or ? 0u : ~m);
      }
      __syncthreads();
      unsigned* sw = a; a = b; b = sw;
    }
    const uint8_t* r8 = (const uint8_t*)a;
    if (lx < tw) {
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int ly = ly0 + 4 * j;
        if (ly < th) out[(size_t)(y0 + ly) * W + x0 + lx] = r8[(halo + ly) * (4 * kSP) + halo + lx];
      }
    }
  }
}

Ellipse make_ellipse(int r) {                              // mask_element's rule (mask_post.hip) at odd sides up to 63
  Ellipse el;
  el.r = r;
  const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
  for (int i = 0; i <= 2 * kMaxR; ++i) {
    const int dy = i - r;
    el.dx[i] = i <= 2 * r ? (unsigned char)(int)__builtin_rint(r * __builtin_sqrt((r * r - dy * dy) * inv_r2)) : 0;
  }
  return el;
}

}  // namespace

int enhance_gauss_taps(int blur_kernel, float* out) {
  if (!out || blur_kernel < 0 || blur_kernel > 2 * kMaxR + 1) return 0;
  const int k = blur_kernel | 1;                           // an even size is raised by one; 0 (no blur) is the one-tap kernel {1}
  static const float small[4][7] = {{1.f}, {0.25f, 0.5f, 0.25f}, {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                    {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
  if (k <= 7) {
    for (int i = 0; i < k; ++i) out[i] = small[k / 2][i];
    return k;
  }
  const double sigma = ((k - 1) * 0.5 - 1) * 0.3 + 0.8, scale2x = -0.5 / (sigma * sigma);
  double t[2 * kMaxR + 1], sum = 0;
  for (int i = 0; i < k; ++i) {
    const double x = i - (k - 1) * 0.5;
    t[i] = std::exp(scale2x * x * x);
    sum += t[i];
  }
  for (int i = 0; i < k; ++i) out[i] = (float)(t[i] / sum);
  return k;
}

size_t enhance_workspace_bytes(int N, size_t mask_bytes) { return rup256((size_t)N * sizeof(Rec)) + 2 * rup256(mask_bytes); }

hipError_t launch_enhance_masks_ragged(const uint8_t* in, uint8_t* out, size_t mask_bytes, const ImageDesc* descs, int N, int expand_pixels,
                                       int blur_kernel, int smooth_iterations, long long max_pixels, long long* stats, void* ws,
                                       hipStream_t st) {
  Rec* recs = (Rec*)ws;
  uint8_t* a = (uint8_t*)ws + rup256((size_t)N * sizeof(Rec));
  uint8_t* b = a + rup256(mask_bytes);
  float full[2 * kMaxR + 1];
  Taps tp;
  const int k = enhance_gauss_taps(blur_kernel, full);
  if (k < 1) return hipErrorInvalidValue;
  tp.r = k / 2;
  for (int i = 0; i <= kMaxR; ++i) tp.t[i] = i <= tp.r ? full[tp.r + i] : 0.f;
  // tiles of an h x w image: at most h*w / 4096 + (h + w) / 64 + 1; the grid covers an image of ordinary proportions (h + w up to
  // 3 sqrt(max_pixels)) in one turn, the kernels stride over the tiles of a narrower one
  long long root = 1;
  while (root * root < max_pixels) root <<= 1;
  long long gx = max_pixels / (kT * kT) + 3 * root / kT + 1;
  if (gx > 65536) gx = 65536;
  long long cx = (max_pixels + kThreads * 16 - 1) / (kThreads * 16);
  if (cx > 65536) cx = 65536;
  const dim3 tiles((unsigned)gx, (unsigned)N), counts((unsigned)cx, (unsigned)N), block(kThreads);

  const Ellipse e7 = make_ellipse(3), e5 = make_ellipse(2), eg = make_ellipse(expand_pixels);
  if (e5.dx[0] != 0 || e5.dx[1] != 2 || e5.dx[2] != 2 || e5.dx[3] != 2 || e5.dx[4] != 0) return hipErrorInvalidValue;      // me_smooth's E(5,5)

  hipLaunchKernelGGL(me_prep, dim3((N + kThreads - 1) / kThreads), block, 0, st, descs, recs, stats, N, (long long)mask_bytes, max_pixels);
  UWM_CHK(hipGetLastError());
  if (stats) hipLaunchKernelGGL(me_count, counts, block, 0, st, in, recs, stats, 0);
  hipLaunchKernelGGL(me_morph<true>, tiles, block, 0, st, in, a, recs, e7);
  hipLaunchKernelGGL(me_morph<false>, tiles, block, 0, st, (const uint8_t*)a, b, recs, e7);
  UWM_CHK(hipGetLastError());
  uint8_t* cur = b;
  uint8_t* oth = a;
  if (expand_pixels > 0) {                                 // (a 1 x 1 element is the identity)
    hipLaunchKernelGGL(me_morph<true>, tiles, block, 0, st, (const uint8_t*)cur, oth, recs, eg);
    uint8_t* t = cur; cur = oth; oth = t;
  }
  hipLaunchKernelGGL(me_blur, tiles, block, 0, st, (const uint8_t*)cur, smooth_iterations ? oth : out, recs, tp);
  UWM_CHK(hipGetLastError());
  { uint8_t* t = cur; cur = oth; oth = t; }
  for (int left = smooth_iterations; left > 0;) {          // kSR rounds of open + close E(5,5) per launch
    const int rounds = left < kSR ? left : kSR;
    left -= rounds;
    hipLaunchKernelGGL(me_smooth, tiles, block, 0, st, (const uint8_t*)cur, left ? oth : out, recs, rounds);
    uint8_t* t = cur; cur = oth; oth = t;
  }
  UWM_CHK(hipGetLastError());
  if (stats) hipLaunchKernelGGL(me_count, counts, block, 0, st, (const uint8_t*)out, recs, stats, 1);
  return hipGetLastError();
}

}  // namespace uwm
