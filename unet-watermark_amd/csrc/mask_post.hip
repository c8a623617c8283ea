// Mask post-processing on the device: the reference's WatermarkPredictor._optimize_mask (binary morphology, 8-connected
// components, selection by area) for uint8 {0,255} masks [N][H][W].  DESIGN.md §8b is the specification; every result is
// exact (integer operations only) and independent of the schedule.
//
// Morphology runs on bit planes: a mask is packed to 1 bit per pixel (bit b of word k of a row = pixel x = 64k + b, row pitch
// WP = ceil(W / 64) words, padding bits always 0), so a 768x1024 mask is 96 KB and every pass of a pipeline stays in L2.  A
// structuring element row is a horizontal run, so a pass is, per output word, an OR / AND over the element's rows of the
// run-dilated (run-eroded) neighbour words.  Pixels outside the image are ignored: 0 for a dilation, 1 for an erosion.
//
// Components: union-find over the pixels with integer atomicMin.  A label array holds parent + 1 (0 = background); a parent is
// never greater than its child, so every find / union chain strictly descends and ends by its own progress, and the root of a
// finished tree is the component's smallest linear index — its first pixel in raster order, the id the specification defines.
// The phases that need a global order are separate launches (init, merge, compress + areas, largest, select + write): no
// grid-wide barrier, no wait on another workgroup.
//
// Every kernel takes its geometry from a source G: Uniform (the [N][H][W] block: image n is H x W at n * H * W) or Ragged (one
// record per image that mp_ragged_prep derives from the descriptors in device memory: validated h and w, the mask offset, the
// offset of the image's bit planes as a prefix sum; h == 0 marks a misfit, whose workgroups leave at once).  Labels and areas of
// a ragged image lie at its mask offset in arrays of mask_bytes ints, values image-local as in the uniform case.
#include "uwm_kernels.h"

namespace uwm {

typedef unsigned long long u64;

namespace {

#include "image_common.inc"

constexpr int kThreads = 256;
constexpr int kPer = 8;                    // pixels per thread of the kernels that end in an atomic sum (mp_cc_compress, mp_select)
constexpr int kPix = kPer * kThreads;
constexpr int kCtr = 16;                   // u64 counters per image: one 128-byte line each, so images do not share an atomic's line

struct Img {                   // one image as a kernel sees it
  int H, W, WP;                // WP = ceil(W / 64): words per row of a bit plane
  size_t pix, word;            // where its pixels (mask bytes, labels, areas) and its bit-plane words begin
};
struct Rec {                   // ragged: one per image, written by mp_ragged_prep; h == 0: misfit
  long long off, word;
  int h, w;
};
struct Uniform {
  static constexpr bool kRagged = false;
  int H, W;
  __device__ __forceinline__ bool get(unsigned n, Img& g) const {
    g.H = H; g.W = W; g.WP = (W + 63) / 64;
    g.pix = (size_t)n * H * W; g.word = (size_t)n * H * g.WP;
    return true;
  }
};
struct Ragged {
  static constexpr bool kRagged = true;
  const Rec* recs;
  __device__ __forceinline__ bool get(unsigned n, Img& g) const {
    const Rec r = recs[n];
    g.H = r.h; g.W = r.w; g.WP = (r.w + 63) / 64;
    g.pix = (size_t)r.off; g.word = (size_t)r.word;
    return r.h != 0;
  }
};

__device__ __forceinline__ u64 valid_bits(int k, int W) {
  const int rem = W - 64 * k;
  return rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
}

// ---------------------------------------------------------------- pack / unpack
// one wave per group of 4 words: lane l reads pixel 64k + l, the ballot is the word
// (the word kernels stride over the grid: the uniform grid covers every word in one turn, a ragged grid is sized for an image of
// ordinary proportions and a very narrow one takes more turns)
template <class G>
__global__ void __launch_bounds__(kThreads) mp_pack(const uint8_t* __restrict__ in, u64* __restrict__ bits, G geo) {
  Img g;
  if (!geo.get(blockIdx.y, g)) return;
  const int H = g.H, W = g.W, WP = g.WP;
  const int lane = threadIdx.x & 63;
  const unsigned nwords = (unsigned)H * WP;
  const uint8_t* img = in + g.pix;
  u64* out = bits + g.word;
  for (unsigned w0 = (blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 4u; w0 < nwords; w0 += gridDim.x * (kThreads / 64) * 4u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned w = w0 + i;
      if (w >= nwords) break;                     // uniform in the wave
      const int y = w / WP, k = w % WP, x = 64 * k + lane;
      const bool fg = x < W && img[(size_t)y * W + x] > 127;
      const u64 word = __ballot(fg);
      if (lane == 0) out[w] = word;
    }
  }
}

__global__ void __launch_bounds__(kThreads) mp_unpack(const u64* __restrict__ bits, uint8_t* __restrict__ out, int H, int W, int WP) {
  const unsigned p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= (unsigned)H * W) return;
  const int y = p / W, x = p % W;
  const u64 word = bits[((size_t)blockIdx.y * H + y) * WP + (x >> 6)];
  out[(size_t)blockIdx.y * H * W + p] = (word >> (x & 63)) & 1 ? 255 : 0;
}

// ---------------------------------------------------------------- one morphology pass on bit planes
struct MorphEl {               // element rows as runs of column offsets [lo, hi] from the anchor (lo > hi: empty row)
  int kh, ay;
  signed char lo[15], hi[15];
};

template <bool DIL, class G>
__global__ void __launch_bounds__(kThreads) mp_morph(const u64* __restrict__ src, u64* __restrict__ dst, const u64* __restrict__ orw,
                                                     G geo, MorphEl el) {
  Img g;
  if (!geo.get(blockIdx.y, g)) return;
  const int H = g.H, W = g.W, WP = g.WP;
  const unsigned nwords = (unsigned)H * WP;
  const u64* plane = src + g.word;
  const u64 outside = DIL ? 0ull : ~0ull;
  for (unsigned idx = blockIdx.x * kThreads + threadIdx.x; idx < nwords; idx += gridDim.x * kThreads) {
    const int y = idx / WP, k = idx % WP;
    u64 acc = outside;
    for (int i = 0; i < el.kh; ++i) {
      const int yy = y + i - el.ay, lo = el.lo[i], hi = el.hi[i];
      if (lo > hi || yy < 0 || yy >= H) continue;          // a row outside the image is ignored
      const u64* row = plane + (size_t)yy * WP;
      u64 cur = row[k], prev = outside, next = outside;
      if (k > 0) prev = row[k - 1];
      if (k + 1 < WP) next = row[k + 1];
      if (!DIL) {                                          // the padding bits of a row's last word lie outside the image
        cur |= ~valid_bits(k, W);
        if (k + 1 < WP) next |= ~valid_bits(k + 1, W);
      }
      u64 r = outside;
      for (int dx = lo; dx <= hi; ++dx) {                  // bit b of v = source pixel 64k + b + dx
        u64 v = cur;
        if (dx > 0) v = (cur >> dx) | (next << (64 - dx));
        else if (dx < 0) v = (cur << -dx) | (prev >> (64 + dx));
        r = DIL ? (r | v) : (r & v);
      }
      acc = DIL ? (acc | r) : (acc & r);
    }
    acc &= valid_bits(k, W);
    if (orw) acc |= orw[g.word + idx];
    dst[g.word + idx] = acc;
  }
}

// ---------------------------------------------------------------- components
// (the union-find is image_common.inc's, labels = parent + 1)
__device__ __forceinline__ bool bit_at(const u64* plane, int WP, int y, int x) {
  return (plane[(size_t)y * WP + (x >> 6)] >> (x & 63)) & 1;
}

// labels = start of the pixel's run inside its 64-pixel word (+ 1), areas = 0; the per-image counters are cleared
template <class G>
__global__ void __launch_bounds__(kThreads) mp_cc_init(const u64* __restrict__ bits, int* __restrict__ labels, int* __restrict__ areas,
                                                       u64* __restrict__ counters, G geo) {
  const unsigned p = blockIdx.x * kThreads + threadIdx.x;
  if (p < (G::kRagged ? 8 : 4)) counters[(size_t)blockIdx.y * kCtr + p] = 0;
  Img g;
  if (!geo.get(blockIdx.y, g)) return;
  const int H = g.H, W = g.W, WP = g.WP;
  if (p >= (unsigned)H * W) return;
  const int y = p / W, x = p % W, b = x & 63;
  const u64 word = bits[g.word + (size_t)y * WP + (x >> 6)];
  int l = 0;
  if ((word >> b) & 1) {
    const u64 gaps = ~word & ((1ull << b) - 1ull);       // background bits below b; the run starts above the highest
    const int start = gaps ? 64 - __clzll((long long)gaps) : 0;
    l = (int)p - b + start + 1;
  }
  labels[g.pix + p] = l;
  areas[g.pix + p] = 0;
}

// joins across word boundaries and between rows (cc_join, 8-connected)
template <class G>
__global__ void __launch_bounds__(kThreads) mp_cc_merge(const u64* __restrict__ bits, int* __restrict__ labels, G geo) {
  Img g;
  if (!geo.get(blockIdx.y, g)) return;
  const int H = g.H, W = g.W, WP = g.WP;
  const unsigned p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= (unsigned)H * W) return;
  const int y = p / W, x = p % W;
  const u64* plane = bits + g.word;
  if (!bit_at(plane, WP, y, x)) return;
  cc_join<true, 1>(labels + g.pix, (int)p, x, y, W, [&](int dy, int dx) { return bit_at(plane, WP, y + dy, x + dx); }, (x & 63) == 0);
}

// labels <- root + 1, areas[root] += pixel count.  A workgroup covers kPix consecutive pixels; each wave sums the lanes that share
// the root of its first foreground lane, the workgroup merges equal roots in LDS, so a large component costs one atomic add per
// workgroup, not one per pixel (a single address takes only so many atomics per microsecond).
template <class G>
__global__ void __launch_bounds__(kThreads) mp_cc_compress(int* __restrict__ labels, int* __restrict__ areas, G geo) {
  __shared__ int s_root[kPer * kThreads / 64], s_cnt[kPer * kThreads / 64];
  Img g;
  if (!geo.get(blockIdx.y, g)) return;                   // (uniform in the workgroup, like the next line)
  const int H = g.H, W = g.W;
  if ((size_t)blockIdx.x * kPix >= (size_t)H * W) return;
  int* lab = labels + g.pix;
  int* ar = areas + g.pix;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const unsigned p = blockIdx.x * kPix + i * kThreads + threadIdx.x;
    int r = -1;
    if (p < (unsigned)H * W && ld_label(lab + p) != 0) {
      r = uf_find<1>(lab, (int)p);
      st_label(lab + p, r + 1);
    }
    const u64 fg = __ballot(r >= 0);
    int r0 = -1, cnt = 0;
    if (fg) {                                            // uniform in the wave
      r0 = __shfl(r, __ffsll((long long)fg) - 1);
      cnt = __popcll(__ballot(r == r0));
      if (r >= 0 && r != r0) atomicAdd(ar + r, 1);       // the lanes of other components (borders between components are short)
    }
    if (lane == 0) { s_root[i * (kThreads / 64) + wave] = r0; s_cnt[i * (kThreads / 64) + wave] = cnt; }
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < kPer * kThreads / 64 && s_root[j] >= 0) {      // the first entry of each root adds the sum of all its entries
    int total = 0;
    bool first = true;
    for (int k = 0; k < kPer * kThreads / 64; ++k)
      if (s_root[k] == s_root[j]) { if (k < j) first = false; total += s_cnt[k]; }
    if (first) atomicAdd(ar + s_root[j], total);
  }
}

// smallest area a component is kept from, where the rule is a threshold.  Watermark: 201 holds only while the largest is below 500
__device__ __forceinline__ int keep_from(int mask_type) { return mask_type == 0 ? 201 : mask_type == 1 ? 51 : mask_type == 2 ? 101 : 1; }

// counters[n][kCtr] = {components, max of (area << 32 | ~id), foreground of the output, [ragged: components with area >=
// keep_from, the largest such area,] unused ...}
template <class G>
__global__ void __launch_bounds__(kThreads) mp_cc_largest(const int* __restrict__ labels, const int* __restrict__ areas,
                                                          u64* __restrict__ counters, G geo, int mask_type) {
  Img g;
  if (!geo.get(blockIdx.y, g)) return;
  const unsigned p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= (unsigned)g.H * g.W) return;
  if (labels[g.pix + p] != (int)p + 1) return;           // roots only
  u64* c = counters + (size_t)blockIdx.y * kCtr;
  const int area = areas[g.pix + p];
  atomicAdd(c, 1ull);
  atomicMax(c + 1, ((u64)(unsigned)area << 32) | (unsigned)~p);
  if (G::kRagged && area >= keep_from(mask_type)) {
    atomicAdd(c + 3, 1ull);
    atomicMax(c + 4, (u64)area);
  }
}

template <class G>
__global__ void __launch_bounds__(kThreads) mp_select(const int* __restrict__ labels, const int* __restrict__ areas, u64* __restrict__ counters,
                                                      uint8_t* __restrict__ out, G geo, int mask_type) {
  __shared__ int s_kept[kThreads / 64];
  Img g;
  if (!geo.get(blockIdx.y, g)) return;                   // (uniform in the workgroup, like the next line)
  const int H = g.H, W = g.W;
  if ((size_t)blockIdx.x * kPix >= (size_t)H * W) return;
  const size_t base = g.pix;
  const u64 best = counters[(size_t)blockIdx.y * kCtr + 1];
  int kept = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const unsigned p = blockIdx.x * kPix + i * kThreads + threadIdx.x;
    bool keep = false;
    if (p < (unsigned)H * W) {
      const int l = labels[base + p];
      if (l) {
        const int area = areas[base + l - 1];
        if (mask_type == 0)                              // watermark: the largest, or everything above 200 when it is below 500
          keep = (int)(best >> 32) < 500 ? area > 200 : (unsigned)(l - 1) == ~(unsigned)best;
        else
          keep = area >= keep_from(mask_type);           // text: > 50 | mixed: > 100 | none (ragged only): every component
      }
      out[base + p] = keep ? 255 : 0;
    }
    kept += __popcll(__ballot(keep));                    // (the same sum in every lane of the wave)
  }
  if ((threadIdx.x & 63) == 0) s_kept[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {                                // one add per workgroup
    int total = 0;
    for (int k = 0; k < kThreads / 64; ++k) total += s_kept[k];
    if (total) atomicAdd(counters + (size_t)blockIdx.y * kCtr + 2, (u64)total);
  }
}

__global__ void mp_summary(const u64* __restrict__ counters, long long* __restrict__ summary, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const u64 ncomp = counters[(size_t)n * kCtr], best = counters[(size_t)n * kCtr + 1];
  summary[(size_t)n * 4 + 0] = (long long)ncomp;
  summary[(size_t)n * 4 + 1] = (long long)(best >> 32);
  summary[(size_t)n * 4 + 2] = (long long)counters[(size_t)n * kCtr + 2];
  summary[(size_t)n * 4 + 3] = ncomp ? (long long)~(unsigned)best : -1ll;
}

// stats[n][8] of the ragged call (include/uwm.h).  The kept components are the roots the selection keeps: every root from
// keep_from up, except that the watermark type keeps the largest alone once its area reaches 500.
__global__ void mp_ragged_stats(const u64* __restrict__ counters, const Rec* __restrict__ recs, long long* __restrict__ stats, int N,
                                int mask_type) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  long long* s = stats + (size_t)n * 8;
  const Rec r = recs[n];
  if (r.h == 0) {
    for (int i = 0; i < 7; ++i) s[i] = 0;
    s[7] = 1;
    return;
  }
  const u64* c = counters + (size_t)n * kCtr;
  const long long ncomp = (long long)c[0], best = (long long)(c[1] >> 32);
  long long kept = (long long)c[3], kept_area = (long long)c[4];
  if (mask_type == 0 && best >= 500) { kept = 1; kept_area = best; }
  s[0] = ncomp;
  s[1] = best;
  s[2] = (long long)c[2];
  s[3] = ncomp ? (long long)~(unsigned)c[1] : -1ll;
  s[4] = kept;
  s[5] = kept_area;
  s[6] = (long long)r.h * r.w;
  s[7] = 0;
}

// one workgroup: validates every descriptor and lays the images' bit planes out one after the other (prefix sums over N in
// turns of kThreads images).  An image takes part in the sums when its sides, its pixel count and its region are in order; it is
// still a misfit when the rows or the plane words up to and including its own exceed the capacities.
__global__ void __launch_bounds__(kThreads) mp_ragged_prep(const ImageDesc* __restrict__ descs, Rec* __restrict__ recs, int N, long long mask_bytes,
                                                           long long max_pixels, long long rows, long long cap_words) {
  __shared__ long long s_rows[kThreads], s_words[kThreads], s_carry[2];
  const int t = threadIdx.x;
  if (t < 2) s_carry[t] = 0;
  for (int base = 0; base < N; base += kThreads) {
    __syncthreads();
    const int i = base + t;
    Rec r = {0, 0, 0, 0};
    if (i < N) {
      const ImageDesc d = descs[i];
      if (region_ok(d, 1, (size_t)mask_bytes) && (long long)d.h * d.w <= max_pixels) { r.off = d.offset; r.h = d.h; r.w = d.w; }
    }
    const long long my_rows = r.h, my_words = (long long)r.h * ((r.w + 63) / 64);
    s_rows[t] = my_rows;
    s_words[t] = my_words;
    block_scan_incl(s_rows, t, s_words);
    const long long rows_to = s_carry[0] + s_rows[t], words_to = s_carry[1] + s_words[t];
    if (rows_to > rows || words_to > cap_words) r.h = r.w = 0, r.off = 0;
    r.word = r.h ? words_to - my_words : 0;
    if (i < N) recs[i] = r;
    __syncthreads();
    if (t == kThreads - 1) { s_carry[0] = rows_to; s_carry[1] = words_to; }
  }
}

// ---------------------------------------------------------------- host side
struct Layout {                // workspace: three bit planes, labels, areas, per-image counters (each 256-byte aligned)
  size_t plane, labels, areas, counters, total;
};
Layout layout(int N, int H, int W) {
  Layout l;
  const size_t WP = ((size_t)W + 63) / 64;
  l.plane = rup256((size_t)N * H * WP * 8);
  l.labels = 3 * l.plane;
  l.areas = l.labels + rup256((size_t)N * H * W * 4);
  l.counters = l.areas + rup256((size_t)N * H * W * 4);
  l.total = l.counters + rup256((size_t)N * kCtr * 8);
  return l;
}

bool make_el(int shape, int kw, int kh, MorphEl* el) {
  uint8_t k[15 * 15];
  if (mask_element(shape, kw, kh, k)) return false;
  el->kh = kh; el->ay = kh / 2;
  const int ax = kw / 2;
  for (int i = 0; i < kh; ++i) {
    int lo = 1, hi = 0;
    for (int j = 0; j < kw; ++j) if (k[i * kw + j]) { if (lo > hi) lo = j - ax; hi = j - ax; }
    el->lo[i] = (signed char)lo; el->hi[i] = (signed char)hi;
  }
  return true;
}

// a batch as the host launches it: the geometry source and the grids, which cover `pixels` pixels and `words` plane words per image
template <class G>
struct Batch {
  G geo;
  int N;
  size_t pixels, words;
  dim3 per_pixel() const { return dim3((unsigned)((pixels + kThreads - 1) / kThreads), (unsigned)N); }
  dim3 per_kpix() const { return dim3((unsigned)((pixels + kPix - 1) / kPix), (unsigned)N); }
  dim3 per_word() const { return dim3((unsigned)((words + kThreads - 1) / kThreads), (unsigned)N); }
  dim3 per_pack() const { return dim3((unsigned)(((words + 3) / 4 + 3) / 4), (unsigned)N); }      // 4 words per wave, 4 waves per workgroup
};
Batch<Uniform> uniform(int N, int H, int W) { return {{H, W}, N, (size_t)H * W, (size_t)H * ((W + 63) / 64)}; }
// the pixel grids cover the largest image allowed; the word grids an image of max_pixels that is at least 64 wide or, narrower,
// at most 4096 high, and the word kernels stride over the rest
Batch<Ragged> ragged(const Rec* recs, int N, long long max_pixels) {
  return {{recs}, N, (size_t)max_pixels, (size_t)(max_pixels / 64 + (max_pixels < 4096 ? max_pixels : 4096))};
}

template <class G>
hipError_t morph_pass(const u64* src, u64* dst, const u64* orw, const Batch<G>& b, bool dil, const MorphEl& el, hipStream_t st) {
  if (dil) hipLaunchKernelGGL((mp_morph<true, G>), b.per_word(), dim3(kThreads), 0, st, src, dst, orw, b.geo, el);
  else hipLaunchKernelGGL((mp_morph<false, G>), b.per_word(), dim3(kThreads), 0, st, src, dst, orw, b.geo, el);
  return hipGetLastError();
}

// `it` passes of one operation, ping-pong between *cur and *tmp; the result is in *cur afterwards
template <class G>
hipError_t morph_n(u64** cur, u64** tmp, const Batch<G>& b, bool dil, const MorphEl& el, int it, hipStream_t st) {
  for (int i = 0; i < it; ++i) {
    hipError_t e = morph_pass(*cur, *tmp, nullptr, b, dil, el, st);
    if (e != hipSuccess) return e;
    u64* t = *cur; *cur = *tmp; *tmp = t;
  }
  return hipSuccess;
}
template <class G>
hipError_t open_close(u64** cur, u64** tmp, const Batch<G>& b, bool close, int shape, int kw, int kh, int it, hipStream_t st) {
  MorphEl el;
  if (!make_el(shape, kw, kh, &el)) return hipErrorInvalidValue;
  hipError_t e = morph_n(cur, tmp, b, close, el, it, st);
  if (e != hipSuccess) return e;
  return morph_n(cur, tmp, b, !close, el, it, st);
}

template <class G>
hipError_t pack(const uint8_t* in, u64* bits, const Batch<G>& b, hipStream_t st) {
  hipLaunchKernelGGL(mp_pack<G>, b.per_pack(), dim3(kThreads), 0, st, in, bits, b.geo);
  return hipGetLastError();
}

template <class G>
hipError_t components(const u64* bits, int* labels, int* areas, u64* counters, const Batch<G>& b, hipStream_t st) {
  hipLaunchKernelGGL(mp_cc_init<G>, b.per_pixel(), dim3(kThreads), 0, st, bits, labels, areas, counters, b.geo);
  hipLaunchKernelGGL(mp_cc_merge<G>, b.per_pixel(), dim3(kThreads), 0, st, bits, labels, b.geo);
  hipLaunchKernelGGL(mp_cc_compress<G>, b.per_kpix(), dim3(kThreads), 0, st, labels, areas, b.geo);
  return hipGetLastError();
}

// pack -> the type's morphology -> components -> largest -> select + write: what the uniform and the ragged call share.
// a, b, c: three bit planes; the counters are left for the caller's summary
template <class G>
hipError_t optimize(const uint8_t* in, uint8_t* out, const Batch<G>& bt, int mask_type, u64* a, u64* b, u64* c, int* labels, int* areas,
                    u64* counters, hipStream_t st) {
  const int E = 2, R = 0;
  MorphEl el;
  UWM_CHK(pack(in, a, bt, st));
  if (mask_type == 0) {                                   // watermark
    UWM_CHK(open_close(&a, &b, bt, false, E, 3, 3, 1, st));
    UWM_CHK(open_close(&a, &b, bt, true, E, 7, 7, 3, st));
    UWM_CHK(open_close(&a, &b, bt, true, E, 11, 11, 2, st));
    make_el(E, 9, 9, &el);
    UWM_CHK(morph_n(&a, &b, bt, true, el, 2, st));
  } else if (mask_type == 1) {                            // text
    UWM_CHK(open_close(&a, &b, bt, false, E, 2, 2, 1, st));
    UWM_CHK(open_close(&a, &b, bt, true, E, 3, 3, 2, st));
    // the two line closings read the same input (a): c = close(a, 5x1); a = close(a, 1x5) | c
    make_el(R, 5, 1, &el);
    UWM_CHK(morph_pass(a, b, (const u64*)nullptr, bt, true, el, st));
    UWM_CHK(morph_pass(b, c, (const u64*)nullptr, bt, false, el, st));
    make_el(R, 1, 5, &el);
    UWM_CHK(morph_pass(a, b, (const u64*)nullptr, bt, true, el, st));
    UWM_CHK(morph_pass(b, a, c, bt, false, el, st));
    make_el(E, 4, 4, &el);
    UWM_CHK(morph_n(&a, &b, bt, true, el, 1, st));
  } else if (mask_type == 2) {                            // mixed
    UWM_CHK(open_close(&a, &b, bt, false, E, 2, 2, 1, st));
    UWM_CHK(open_close(&a, &b, bt, true, E, 5, 5, 2, st));
    make_el(E, 6, 6, &el);
    UWM_CHK(morph_n(&a, &b, bt, true, el, 1, st));
  }                                                       // (none, ragged only: the binarised plane as it is)
  UWM_CHK(components(a, labels, areas, counters, bt, st));
  hipLaunchKernelGGL(mp_cc_largest<G>, bt.per_pixel(), dim3(kThreads), 0, st, labels, areas, counters, bt.geo, mask_type);
  hipLaunchKernelGGL(mp_select<G>, bt.per_kpix(), dim3(kThreads), 0, st, labels, areas, counters, out, bt.geo, mask_type);
  return hipGetLastError();
}

struct RaggedLayout {          // workspace of the ragged call: records, counters, three bit planes of cap_words, labels, areas
  size_t cap_words, counters, plane0, plane, labels, areas, total;
};
RaggedLayout ragged_layout(int N, size_t mask_bytes, long long rows) {
  RaggedLayout l;
  l.cap_words = mask_bytes / 64 + (size_t)rows;            // sum of h_i * ceil(w_i / 64) <= sum of h_i * w_i / 64 + sum of h_i
  l.counters = rup256((size_t)N * sizeof(Rec));
  l.plane0 = l.counters + rup256((size_t)N * kCtr * 8);
  l.plane = rup256(l.cap_words * 8);
  l.labels = l.plane0 + 3 * l.plane;
  l.areas = l.labels + rup256(mask_bytes * 4);
  l.total = l.areas + rup256(mask_bytes * 4);
  return l;
}

}  // namespace

int mask_element(int shape, int kw, int kh, uint8_t* out) {
  if (!out || kw < 1 || kh < 1 || kw > 15 || kh > 15 || (shape != 0 && shape != 2)) return 1;
  if (shape == 0) {
    for (int i = 0; i < kw * kh; ++i) out[i] = 1;
    return 0;
  }
  // cv2.getStructuringElement(MORPH_ELLIPSE): row i covers c +- round_half_even(c * sqrt((r^2 - dy^2) / r^2))
  const int r = kh / 2, c = kw / 2;
  const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
  for (int i = 0; i < kh; ++i) {
    const int dy = i - r;
    int j1 = 0, j2 = 0;
    if (dy >= -r && dy <= r) {
      const int dx = (int)__builtin_rint(c * __builtin_sqrt((r * r - dy * dy) * inv_r2));     // (default rounding mode: half to even)
      j1 = c - dx > 0 ? c - dx : 0;
      j2 = c + dx + 1 < kw ? c + dx + 1 : kw;
    }
    for (int j = 0; j < kw; ++j) out[i * kw + j] = j >= j1 && j < j2;
  }
  return 0;
}

size_t mask_workspace_bytes(int N, int H, int W) { return layout(N, H, W).total; }

size_t mask_ragged_workspace_bytes(int N, size_t mask_bytes, long long rows) { return ragged_layout(N, mask_bytes, rows).total; }

hipError_t launch_mask_morph(const uint8_t* in, uint8_t* out, int N, int H, int W, int dilate, int shape, int kw, int kh,
                             int iterations, void* ws, hipStream_t st) {
  const Layout l = layout(N, H, W);
  const Batch<Uniform> bt = uniform(N, H, W);
  u64* cur = (u64*)ws;
  u64* tmp = (u64*)((char*)ws + l.plane);
  MorphEl el;
  if (!make_el(shape, kw, kh, &el)) return hipErrorInvalidValue;
  UWM_CHK(pack(in, cur, bt, st));
  UWM_CHK(morph_n(&cur, &tmp, bt, dilate != 0, el, iterations, st));
  hipLaunchKernelGGL(mp_unpack, bt.per_pixel(), dim3(kThreads), 0, st, cur, out, H, W, (W + 63) / 64);
  return hipGetLastError();
}

hipError_t launch_mask_components(const uint8_t* in, int* labels, int* areas, int N, int H, int W, void* ws, hipStream_t st) {
  const Layout l = layout(N, H, W);
  const Batch<Uniform> bt = uniform(N, H, W);
  UWM_CHK(pack(in, (u64*)ws, bt, st));
  return components((u64*)ws, labels, areas, (u64*)((char*)ws + l.counters), bt, st);
}

hipError_t launch_optimize_mask(const uint8_t* in, uint8_t* out, int N, int H, int W, int mask_type, long long* summary, void* ws,
                                hipStream_t st) {
  const Layout l = layout(N, H, W);
  u64* counters = (u64*)((char*)ws + l.counters);
  UWM_CHK(optimize(in, out, uniform(N, H, W), mask_type, (u64*)ws, (u64*)((char*)ws + l.plane), (u64*)((char*)ws + 2 * l.plane),
                  (int*)((char*)ws + l.labels), (int*)((char*)ws + l.areas), counters, st));
  if (summary) hipLaunchKernelGGL(mp_summary, dim3((N + 63) / 64), dim3(64), 0, st, counters, summary, N);
  return hipGetLastError();
}

hipError_t launch_optimize_masks_ragged(const uint8_t* in, uint8_t* out, size_t mask_bytes, const ImageDesc* descs, int N, int mask_type,
                                        long long max_pixels, long long rows, long long* stats, void* ws, hipStream_t st) {
  const RaggedLayout l = ragged_layout(N, mask_bytes, rows);
  Rec* recs = (Rec*)ws;
  u64* counters = (u64*)((char*)ws + l.counters);
  u64* a = (u64*)((char*)ws + l.plane0);
  hipLaunchKernelGGL(mp_ragged_prep, dim3(1), dim3(kThreads), 0, st, descs, recs, N, (long long)mask_bytes, max_pixels, rows,
                     (long long)l.cap_words);
  UWM_CHK(hipGetLastError());
  UWM_CHK(optimize(in, out, ragged(recs, N, max_pixels), mask_type, a, (u64*)((char*)a + l.plane), (u64*)((char*)a + 2 * l.plane),
                  (int*)((char*)ws + l.labels), (int*)((char*)ws + l.areas), counters, st));
  if (stats) hipLaunchKernelGGL(mp_ragged_stats, dim3((N + 63) / 64), dim3(64), 0, st, counters, recs, stats, N, mask_type);
  return hipGetLastError();
}

}  // namespace uwm
