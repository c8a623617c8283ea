// Scoring predicted masks against ground truth on the device: the four region counts (tp, fp, fn, tn) and the three counts of
// Boundary IoU (Cheng et al., CVPR 2021) for a ragged batch of mask pairs in one call.  DESIGN.md §8s is the specification; every
// result is an integer and the same on every run (popcounts summed with integer atomics).
//
// Both masks are binarised (> 127) and packed to bit planes as in mask_post.hip (bit b of word k of a row = pixel 64k + b, pitch
// WP = ceil(W / 64) words, padding bits 0).  The erosion E_d by the (2d+1) x (2d+1) square, everything outside the image unset, is
// separable, and neither half loops over the window:
//   rows     one wave holds a row — one word per lane (ms_pack_erode_rows_narrow: widths up to 3968) or a stretch of it in LDS
//            (ms_pack_erode_rows_wide) — and forms A_L(x) = AND of M[x .. x+L-1], L = 2d + 1, by window doubling: A_2n(x) =
//            A_n(x) & A_n(x + n), then A_L(x) = A_n(x) & A_n(x + L - n) for the rest; the eroded row is A_L shifted by d.
//            ceil(log2 L) + 1 steps at the most, each a funnel shift over the row's words.
//   columns  ms_erode_columns cuts each column of words into segments of L rows and writes the ANDs from the segment's start (p) and
//            to its end (s); E(y) = s(y - d) & p(y + d) (van Herk / Gil-Werman).  Two sweeps over the plane whatever d is.
// ms_count forms E from s and p while it counts, so the eroded planes are never stored.  An image with 2d + 1 above a side has an
// empty erosion and skips both halves; d = 0 skips the boundary part altogether.
//
// Five launches whatever N and the radii are: ms_prep (validates descriptors and radii, lays out the planes, zeroes the counts),
// the two row kernels (each image is served by one and left at once by the other), ms_erode_columns, ms_count.  A misfit's record
// has h == 0 and its workgroups leave at once.
#include "uwm_kernels.h"

namespace uwm {

typedef unsigned long long u64;

namespace {

#include "image_common.inc"

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRadius = 32767;
constexpr int kSpan = 1536;                // words of a row stretch in LDS per wave: its output words and ceil(d / 64) <= 512 on either side
constexpr int kSpanPerLane = kSpan / 64;
constexpr int kPlanes = 6;                 // per mask: the packed plane M, the row-eroded plane (later p), and s

struct Rec {                   // one per image, written by ms_prep; h == 0: misfit
  long long off, word;         // where its bytes begin in both buffers, and its words in every plane
  int h, w, d, erode;          // erode: 0 < 2d + 1 <= min(h, w), so E_d is neither skipped nor empty
};

__device__ __forceinline__ u64 valid_bits(int k, int W) {
  const int rem = W - 64 * k;
  return rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
}

// one workgroup: validates every descriptor and radius and lays the images' planes out one after the other (the rule of
// mp_ragged_prep in mask_post.hip).  An image takes part in the sums when its sides, its pixel count, its region and its radius are
// in order; it is still a misfit when the rows or the plane words up to and including its own exceed the capacities.
__global__ void __launch_bounds__(kThreads) ms_prep(const ImageDesc* __restrict__ descs, const int* __restrict__ radius, Rec* __restrict__ recs,
                                                    long long* __restrict__ counts, int N, long long mask_bytes, long long max_pixels,
                                                    long long rows, long long cap_words) {
  __shared__ long long s_rows[kThreads], s_words[kThreads], s_carry[2];
  const int t = threadIdx.x;
  if (t < 2) s_carry[t] = 0;
  for (int base = 0; base < N; base += kThreads) {
    __syncthreads();
    const int i = base + t;
    Rec r = {0, 0, 0, 0, 0, 0};
    if (i < N) {
      const ImageDesc d = descs[i];
      const int rad = radius[i];
      if (region_ok(d, 1, (size_t)mask_bytes) && (long long)d.h * d.w <= max_pixels && rad >= 0 && rad <= kMaxRadius) {
        r.off = d.offset; r.h = d.h; r.w = d.w; r.d = rad;
      }
    }
    const long long my_rows = r.h, my_words = (long long)r.h * ((r.w + 63) / 64);
    s_rows[t] = my_rows;
    s_words[t] = my_words;
    block_scan_incl(s_rows, t, s_words);
    const long long rows_to = s_carry[0] + s_rows[t], words_to = s_carry[1] + s_words[t];
    if (rows_to > rows || words_to > cap_words) r.h = r.w = r.d = 0, r.off = 0;
    r.word = r.h ? words_to - my_words : 0;
    r.erode = r.h && r.d > 0 && 2 * r.d + 1 <= min(r.h, r.w);
    if (i < N) {
      recs[i] = r;
      for (int j = 0; j < 7; ++j) counts[(size_t)i * 8 + j] = 0;
      counts[(size_t)i * 8 + 7] = r.h ? 0 : 1;
    }
    __syncthreads();
    if (t == kThreads - 1) { s_carry[0] = rows_to; s_carry[1] = words_to; }
  }
}

// bits [64j + sh, 64j + sh + 64) of the n words at buf; words from n on read as 0
__device__ __forceinline__ u64 funnel(const u64* buf, int j, int sh, int n) {
  const int q = j + (sh >> 6), r = sh & 63;
  const u64 a = q < n ? buf[q] : 0ull;
  if (r == 0) return a;
  const u64 b = q + 1 < n ? buf[q + 1] : 0ull;
  return (a >> r) | (b << (64 - r));
}

// buf[j] &= bits of buf at distance sh, for the n words of every wave's stretch.  The whole workgroup comes here with the same n
// and sh: every word is read before any is written.
__device__ __forceinline__ void and_shifted(u64* buf, int n, int sh, int lane) {
  u64 t[kSpanPerLane];
#pragma unroll
  for (int i = 0; i < kSpanPerLane; ++i) {
    const int j = i * 64 + lane;
    if (i * 64 < n) t[i] = j < n ? buf[j] & funnel(buf, j, sh, n) : 0ull;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kSpanPerLane; ++i) {
    const int j = i * 64 + lane;
    if (i * 64 < n && j < n) buf[j] = t[i];
  }
  __syncthreads();
}

// a row with its halo fits one word per lane (ceil(w / 64) + 2 ceil(d / 64) <= 64: every width up to 3968 at d <= 64, 3840 at d <=
// 128): ms_pack_erode_rows_narrow serves it from registers; ms_pack_erode_rows_wide serves the others from LDS
__device__ __forceinline__ bool row_fits_wave(int WP, int hw) { return WP + 2 * hw <= 64; }

// the same funnel over a row held one word per lane (v of lane j = word j; lanes past the row hold 0): every lane of the wave comes here
__device__ __forceinline__ u64 wave_funnel(u64 v, int lane, int sh) {
  const int q = lane + (sh >> 6), r = sh & 63;
  const u64 a = __shfl(v, q & 63, 64), b = __shfl(v, (q + 1) & 63, 64);
  const u64 lo = q < 64 ? a : 0ull, hi = q + 1 < 64 ? b : 0ull;
  return r == 0 ? lo : (lo >> r) | (hi << (64 - r));
}

// Packs both masks and erodes their rows, one row per wave, the row in registers: lane j holds word j - hw of the row, hw =
// ceil(d / 64) (0 without erosion), so bit 64 * hw - d + i of the lanes' words is what output bit i of A_L reads first.  No LDS and
// no barrier: the doubling steps are wave shuffles.  planes: M_pred, R_pred, S_pred, M_truth, R_truth, S_truth, `plane` words apart.
__global__ void __launch_bounds__(kThreads) ms_pack_erode_rows_narrow(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                                      u64* __restrict__ planes, size_t plane, const Rec* __restrict__ recs) {
  const Rec r = recs[blockIdx.y];
  if (r.h == 0) return;
  const int H = r.h, W = r.w, WP = (W + 63) / 64, d = r.d;
  const int hw = r.erode ? (d + 63) / 64 : 0;
  if (!row_fits_wave(WP, hw)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = 2 * d + 1, o = 64 * hw - d;
  for (long long y = (long long)blockIdx.x * kWaves + wave; y < H; y += (long long)gridDim.x * kWaves) {
    const uint8_t* ip = pred + r.off + (size_t)y * W;
    const uint8_t* ig = truth + r.off + (size_t)y * W;
    u64 vp = 0, vg = 0;
#pragma unroll 8
    for (int k = 0; k < WP; ++k) {
      const int x = 64 * k + lane;
      const bool in = x < W;
      const u64 wp = __ballot(in && ip[x] > 127), wg = __ballot(in && ig[x] > 127);
      if (lane == k + hw) { vp = wp; vg = wg; }
    }
    u64* M = planes + r.word + (size_t)y * WP;
    if (lane >= hw && lane < hw + WP) { M[lane - hw] = vp; M[3 * plane + lane - hw] = vg; }
    if (r.erode) {
      int w = 1;
      for (; 2 * w <= L; w *= 2) { vp &= wave_funnel(vp, lane, w); vg &= wave_funnel(vg, lane, w); }
      if (w < L) { vp &= wave_funnel(vp, lane, L - w); vg &= wave_funnel(vg, lane, L - w); }
      const u64 ep = wave_funnel(vp, lane, o), eg = wave_funnel(vg, lane, o);
      if (lane < WP) { M[plane + lane] = ep; M[4 * plane + lane] = eg; }
    }
  }
}

// The same for rows that do not fit a wave.  A work item is kWaves rows by one stretch of C = kSpan - 2 hw output words; wave v
// takes row 4 * group + v.  The stretch in LDS begins hw words before the output words, words outside the row read as 0.
__global__ void __launch_bounds__(kThreads) ms_pack_erode_rows_wide(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                                    u64* __restrict__ planes, size_t plane, const Rec* __restrict__ recs) {
  __shared__ u64 s_buf[kWaves][kSpan];
  const Rec r = recs[blockIdx.y];
  if (r.h == 0) return;
  const int H = r.h, W = r.w, WP = (W + 63) / 64, d = r.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hw = r.erode ? (d + 63) / 64 : 0;
  if (row_fits_wave(WP, hw)) return;
  const int C = kSpan - 2 * hw;
  const int L = 2 * d + 1;
  const u64 groups = ((u64)H + kWaves - 1) / kWaves, chunks = ((u64)WP + C - 1) / C;
  u64* buf = s_buf[wave];
  for (u64 item = blockIdx.x; item < groups * chunks; item += gridDim.x) {
    const long long y = (long long)(item / chunks) * kWaves + wave;
    const int c0 = (int)(item % chunks) * C;
    const int cout = min(C, WP - c0);
    const int n = cout + 2 * hw;
    const bool row = y < H;
    for (int m = 0; m < 2; ++m) {
      const uint8_t* img = (m ? truth : pred) + r.off + (size_t)(row ? y : 0) * W;
      u64* M = planes + (size_t)(3 * m) * plane + r.word + (size_t)(row ? y : 0) * WP;
      u64* R = M + plane;
#pragma unroll 4
      for (int j = 0; j < n; ++j) {
        const int k = c0 - hw + j;
        const long long x = 64ll * k + lane;
        const bool fg = row && k >= 0 && x < W && img[x] > 127;
        const u64 word = __ballot(fg);
        if (lane == 0) {
          buf[j] = word;
          if (row && j >= hw && j < hw + cout) M[k] = word;
        }
      }
      __syncthreads();
      if (r.erode) {
        int w = 1;
        for (; 2 * w <= L; w *= 2) and_shifted(buf, n, w, lane);
        if (w < L) and_shifted(buf, n, L - w, lane);
        const int o = 64 * hw - d;
        if (row)
          for (int j = lane; j < cout; j += 64) R[c0 + j] = funnel(buf, j, o, n);
        __syncthreads();
      }
    }
  }
}

// van Herk / Gil-Werman over the rows of words: one thread per (mask, segment of L rows, word column) writes s downwards from the
// segment's end into the S plane, then p upwards from its start over the row-eroded plane itself.
__global__ void __launch_bounds__(kThreads) ms_erode_columns(u64* __restrict__ planes, size_t plane, const Rec* __restrict__ recs) {
  const Rec r = recs[blockIdx.y];
  if (r.h == 0 || !r.erode) return;
  const int H = r.h, WP = (r.w + 63) / 64, L = 2 * r.d + 1;
  const u64 per_mask = (u64)((H + L - 1) / L) * WP;
  for (u64 t = (u64)blockIdx.x * kThreads + threadIdx.x; t < 2 * per_mask; t += (u64)gridDim.x * kThreads) {
    const int m = t >= per_mask;
    const u64 rem = t - m * per_mask;
    const int k = (int)(rem % WP);
    const long long y0 = (long long)(rem / WP) * L, y1 = min((long long)H, y0 + L);
    u64* R = planes + (size_t)(3 * m + 1) * plane + r.word + k;
    u64* S = R + plane;
    u64 acc = ~0ull;
    for (long long y = y1 - 1; y >= y0; --y) { acc &= R[(size_t)y * WP]; S[(size_t)y * WP] = acc; }
    acc = ~0ull;
    for (long long y = y0; y < y1; ++y) { acc &= R[(size_t)y * WP]; R[(size_t)y * WP] = acc; }
  }
}

// counts[n][0..6] += the popcounts over the image's words (include/uwm.h); E_d(y) = s(y - d) & p(y + d) inside the image, else 0
__global__ void __launch_bounds__(kThreads) ms_count(const u64* __restrict__ planes, size_t plane, const Rec* __restrict__ recs,
                                                     long long* __restrict__ counts) {
  __shared__ unsigned s_sum[kWaves][7];
  const Rec r = recs[blockIdx.y];
  if (r.h == 0) return;
  const int H = r.h, W = r.w, WP = (W + 63) / 64, d = r.d;
  const u64 nwords = (u64)H * WP;
  const u64* MP = planes + r.word;
  const u64* MG = MP + 3 * plane;
  unsigned c[7] = {0, 0, 0, 0, 0, 0, 0};
  for (u64 i = (u64)blockIdx.x * kThreads + threadIdx.x; i < nwords; i += (u64)gridDim.x * kThreads) {
    const long long y = (long long)(i / WP);
    const int k = (int)(i % WP);
    const u64 p = MP[i], g = MG[i], v = valid_bits(k, W);
    c[0] += __popcll(p & g);
    c[1] += __popcll(p & ~g);
    c[2] += __popcll(~p & g);
    c[3] += __popcll(~p & ~g & v);
    if (d > 0) {
      u64 ep = 0, eg = 0;
      if (r.erode && y - d >= 0 && y + d < H) {
        const size_t lo = (size_t)(y - d) * WP + k, hi = (size_t)(y + d) * WP + k;
        ep = MP[2 * plane + lo] & MP[plane + hi];
        eg = MG[2 * plane + lo] & MG[plane + hi];
      }
      const u64 bp = p & ~ep, bg = g & ~eg;
      c[4] += __popcll(bp & bg);
      c[5] += __popcll(bp);
      c[6] += __popcll(bg);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    unsigned v = c[j];
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    if (lane == 0) s_sum[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    u64 v = 0;
    for (int w = 0; w < kWaves; ++w) v += s_sum[w][threadIdx.x];
    if (v) atomicAdd((u64*)counts + (size_t)blockIdx.y * 8 + threadIdx.x, v);
  }
}

struct ScoreLayout {           // workspace: records, then kPlanes bit planes of cap_words (each 256-byte aligned)
  size_t cap_words, plane0, plane, total;
};
ScoreLayout score_layout(int N, size_t mask_bytes, long long rows) {
  ScoreLayout l;
  l.cap_words = mask_bytes / 64 + (size_t)rows;            // sum of h_i * ceil(w_i / 64) <= sum of h_i * w_i / 64 + sum of h_i
  l.plane0 = rup256((size_t)N * sizeof(Rec));
  l.plane = rup256(l.cap_words * 8);
  l.total = l.plane0 + kPlanes * l.plane;
  return l;
}

unsigned grid_for(size_t work, size_t per_block, unsigned most) {
  const size_t g = (work + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : g > most ? most : g);
}

}  // namespace

size_t score_masks_workspace_bytes(int N, size_t mask_bytes, long long rows) { return score_layout(N, mask_bytes, rows).total; }

hipError_t launch_score_masks_ragged(const uint8_t* pred, const uint8_t* truth, size_t mask_bytes, const ImageDesc* descs, const int* radius,
                                     int N, long long max_pixels, long long rows, long long* counts, void* ws, hipStream_t st) {
  const ScoreLayout l = score_layout(N, mask_bytes, rows);
  Rec* recs = (Rec*)ws;
  u64* planes = (u64*)((char*)ws + l.plane0);
  const size_t plane = l.plane / 8;
  // the grids cover an image of max_pixels that is at least 64 wide or, narrower, at most 4096 high (as mask_post.hip's word grids);
  // every kernel strides over the rest
  const size_t words = (size_t)(max_pixels / 64 + (max_pixels < 4096 ? max_pixels : 4096));
  hipLaunchKernelGGL(ms_prep, dim3(1), dim3(kThreads), 0, st, descs, radius, recs, counts, N, (long long)mask_bytes, max_pixels, rows,
                     (long long)l.cap_words);
  UWM_CHK(hipGetLastError());
  const dim3 rows_grid(grid_for(words, 32, 2048), (unsigned)N);
  hipLaunchKernelGGL(ms_pack_erode_rows_narrow, rows_grid, dim3(kThreads), 0, st, pred, truth, planes, plane, recs);
  UWM_CHK(hipGetLastError());
  // a row that does not fit a wave is at least 1921 pixels wide (2d + 1 <= w bounds its halo by half its words), so an image of
  // max_pixels has few of them; the kernel strides over whatever the grid does not cover
  const dim3 wide_grid(grid_for((size_t)max_pixels / 1921 + 1, kWaves, 2048), (unsigned)N);
  hipLaunchKernelGGL(ms_pack_erode_rows_wide, wide_grid, dim3(kThreads), 0, st, pred, truth, planes, plane, recs);
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(ms_erode_columns, dim3(grid_for(words, 2 * kThreads, 1024), (unsigned)N), dim3(kThreads), 0, st, planes, plane, recs);
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(ms_count, dim3(grid_for(words, 4 * kThreads, 1024), (unsigned)N), dim3(kThreads), 0, st, planes, plane, recs, counts);
  return hipGetLastError();
}

}  // namespace uwm
