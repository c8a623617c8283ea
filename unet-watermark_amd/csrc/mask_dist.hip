// Exact Euclidean distance transforms of ragged mask batches and the surface distances of mask pairs built on them (Hausdorff, its
// 95th percentile, average surface distance, covering radius).  DESIGN.md §8u and include/uwm.h are the specification; squared
// distances are integers, so every entry of a record is exact and the same on every run.
//
// D2(M)[y][x] = min over the set pixels (y', x') of M of (y - y')^2 + (x - x')^2 is separable (Meijster, Roerdink, Hesselink 2000):
//   columns  md_columns: one thread per column; g[y][x] = the vertical distance to the nearest set pixel of column x (kInf: none), a
//            scan downwards that also decides which pixels are sources (the mask, or its 4-neighbour border), and a scan upwards.
//   rows     md_rows: D2[y][x] = min over x' of (x - x')^2 + g[y][x']^2, the lower envelope of parabolas.  One lane per row, one
//            wave per 64 rows: the forward scan builds the envelope as a stack of (apex column, first column it wins) pairs, the
//            backward scan reads the distances off it.  O(W) per row, 32-bit multiplies and one 32-bit division per column.  g and
//            D2 pass through a 64 x 64 LDS tile, so global reads and writes run along rows while every lane walks its own row; the
//            stack of row y keeps entry q at [q * H + y], so lanes on consecutive rows touch consecutive words.
// Every per-pixel array (g, the stacks, the D2 maps) is indexed like the masks, by descs[i].offset + y * w + x, so a plane of
// mask_bytes entries holds whatever batch the descriptors describe and no layout pass is needed.
//
// uwm_edt_ragged: md_prep, md_columns, md_rows: three launches.  uwm_surface_distances_ragged: md_prep, md_columns and md_rows once
// each for the three transforms of a pair (of the truth's border, of the prediction's border, of the prediction: blockIdx.z),
// md_gather (border counts, maxima with integer atomics, sqrt sums as per-workgroup partials), md_begin (ranks, the sums of the
// partials in a fixed order), then four rounds of md_hist / md_step: a radix select, eight bits a round, of the two order
// statistics among the border distances.  Thirteen launches whatever N and the masks hold.  A misfit's record has h == 0 and its
// workgroups leave at once.
#include "uwm_kernels.h"

namespace uwm {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;

namespace {

#include "image_common.inc"

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSide = 32768;
constexpr int kInf = 65535;                                // g of a column without a source: kInf^2 is above every real D2
constexpr long long kInf2 = (long long)kInf * kInf;
constexpr int kNone = 2147483647;                          // UWM_EDT_NONE
constexpr int kTile = 64;
constexpr int kRowBlocks = 64;                             // most workgroups (of one wave) per image and transform in md_rows
constexpr int kColBlocks = 16;                             // most workgroups per image and transform in md_columns
constexpr int kPixBlocks = 64;                             // workgroups per image in md_gather and md_hist at the most; partials per image
constexpr int kAcc = 8;                                    // per image: 0 |dP|, 1 |dG|, 2 max a, 3 max b, 4 cover (-1: G empty)
constexpr int kSel = 8;                                    // per image: 0, 1 prefixes of v[lo], v[hi]; 2, 3 their ranks left; 4 active; 5 rem

struct Rec {                   // one per image, written by md_prep; h == 0: misfit
  long long off;
  int h, w;
};

// one workgroup: validates every descriptor (the rule of ms_prep in mask_score.hip with sides up to 32768 and no radius), zeroes the
// accumulators of the surface call (null for the transform alone)
__global__ void __launch_bounds__(kThreads) md_prep(const ImageDesc* __restrict__ descs, Rec* __restrict__ recs, long long* __restrict__ acc,
                                                    long long* __restrict__ sel, u64* __restrict__ hist, int N, long long mask_bytes,
                                                    long long max_pixels, long long rows, long long cap_words) {
  __shared__ long long s_rows[kThreads], s_words[kThreads], s_carry[2];
  const int t = threadIdx.x;
  if (t < 2) s_carry[t] = 0;
  for (int base = 0; base < N; base += kThreads) {
    __syncthreads();
    const int i = base + t;
    Rec r = {0, 0, 0};
    if (i < N) {
      const ImageDesc d = descs[i];
      if (region_ok(d, 1, (size_t)mask_bytes, 1, kMaxSide) && (long long)d.h * d.w <= max_pixels) { r.off = d.offset; r.h = d.h; r.w = d.w; }
    }
    const long long my_rows = r.h, my_words = (long long)r.h * ((r.w + 63) / 64);
    s_rows[t] = my_rows;
    s_words[t] = my_words;
    block_scan_incl(s_rows, t, s_words);
    const long long rows_to = s_carry[0] + s_rows[t], words_to = s_carry[1] + s_words[t];
    if (rows_to > rows || words_to > cap_words) r.h = r.w = 0, r.off = 0;
    if (i < N) {
      recs[i] = r;
      if (acc) {
        for (int j = 0; j < kAcc; ++j) acc[(size_t)i * kAcc + j] = j == 4 ? -1 : 0;
        for (int j = 0; j < kSel; ++j) sel[(size_t)i * kSel + j] = 0;
      }
    }
    __syncthreads();
    if (t == kThreads - 1) { s_carry[0] = rows_to; s_carry[1] = words_to; }
  }
  if (hist)
    for (size_t j = t; j < (size_t)N * 512; j += kThreads) hist[j] = 0;
}

// is pixel (y, x) of the h x w mask m (> 127 is set) a border pixel: set, with a 4-neighbour that is unset or outside the image
__device__ __forceinline__ bool border_at(const uint8_t* __restrict__ m, int H, int W, int y, int x) {
  const size_t k = (size_t)y * W + x;
  if (m[k] <= 127) return false;
  if (y == 0 || x == 0 || y == H - 1 || x == W - 1) return true;
  return m[k - 1] <= 127 || m[k + 1] <= 127 || m[k - W] <= 127 || m[k + W] <= 127;
}

// blockIdx.z of the surface call -> the mask its transform starts from, and whether from its border
__device__ __forceinline__ const uint8_t* source_of(const uint8_t* pred, const uint8_t* truth, int surface, int z, bool& border) {
  border = surface && z < 2;
  return surface && z == 0 ? truth : pred;
}

__global__ void __launch_bounds__(kThreads) md_columns(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, int surface,
                                                       u16* __restrict__ g, size_t plane, const Rec* __restrict__ recs) {
  const Rec r = recs[blockIdx.y];
  if (r.h == 0) return;
  const int H = r.h, W = r.w;
  bool border;
  const uint8_t* m = source_of(pred, truth, surface, blockIdx.z, border) + r.off;
  u16* gc = g + (size_t)blockIdx.z * plane + r.off;
  for (int x = blockIdx.x * kThreads + threadIdx.x; x < W; x += gridDim.x * kThreads) {
    int d = kInf;
    bool up = false, cur = m[x] > 127;
    for (int y = 0; y < H; ++y) {
      const size_t k = (size_t)y * W + x;
      const bool dn = y + 1 < H && m[k + W] > 127;
      bool s = cur;
      if (border && s && up && dn) s = !(x > 0 && x + 1 < W && m[k - 1] > 127 && m[k + 1] > 127);
      d = s ? 0 : d == kInf ? kInf : d + 1;
      gc[k] = (u16)d;
      up = cur; cur = dn;
    }
    d = kInf;
    for (int y = H - 1; y >= 0; --y) {
      const size_t k = (size_t)y * W + x;
      const int v = gc[k];
      d = v == 0 ? 0 : d == kInf ? kInf : d + 1;
      if (d < v) gc[k] = (u16)d;
    }
  }
}

// One wave per workgroup.  Lane l serves row 64 * group + l.  The stack's top entry and the one below it are in registers: apex
// column s, the first column t at which it wins, and g(s)^2 (65535^2 fits 32 bits, a sum of two squares takes 64); every entry is
// also in memory, as s | t << 16 (both below 32768) in `stack` and g(s) in `sg`, so a pop only has to fetch the entry that becomes
// the one below the top, which is needed at the next pop at the earliest.
struct Apex { int s, t; u32 g2; };
__device__ __forceinline__ u64 height_at(int x, const Apex& a) { const int d = x - a.s; return (u64)(u32)(d * d) + a.g2; }
__device__ __forceinline__ Apex load_apex(const u32* stk, const u16* sg, size_t at) {
  const u32 e = stk[at], gs = sg[at];
  return Apex{(int)(e & 0xffff), (int)(e >> 16), gs * gs};
}

__global__ void __launch_bounds__(64) md_rows(const u16* __restrict__ g, u32* __restrict__ stack, u16* __restrict__ stack_g, size_t plane,
                                              int* __restrict__ d2, size_t d2_plane, const Rec* __restrict__ recs) {
  __shared__ int tile[kTile][kTile + 1];
  const Rec r = recs[blockIdx.y];
  if (r.h == 0) return;
  const int H = r.h, W = r.w, lane = threadIdx.x;
  const u16* gi = g + (size_t)blockIdx.z * plane + r.off;
  u32* si = stack + (size_t)blockIdx.z * plane + r.off;
  u16* sgi = stack_g + (size_t)blockIdx.z * plane + r.off;
  int* di = d2 + (size_t)blockIdx.z * d2_plane + r.off;
  const int groups = (H + kTile - 1) / kTile, chunks = (W + kTile - 1) / kTile;
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int y0 = grp * kTile, y = y0 + lane;
    const bool valid = y < H;
    u32* stk = si + (valid ? y : 0);
    u16* sg = sgi + (valid ? y : 0);
    int q = -1;
    Apex top = {0, 0, 0}, below = {0, 0, 0};                       // below: entry q - 1, held while q >= 1
    for (int c0 = 0; c0 < chunks; ++c0) {
      const int x0 = c0 * kTile, nx = min(kTile, W - x0);
      __syncthreads();
      for (int rr = 0; rr < kTile; ++rr)
        tile[rr][lane] = (y0 + rr < H && lane < nx) ? gi[(size_t)(y0 + rr) * W + x0 + lane] : kInf;
      __syncthreads();
      if (valid) {
        for (int c = 0; c < nx; ++c) {
          const int u = x0 + c;
          const u32 gu = (u32)tile[lane][c], gu2 = gu * gu;
          const Apex cand = {u, 0, gu2};
          while (q >= 0 && height_at(top.t, top) > height_at(top.t, cand)) {      // apexes that column u beats where they begin to win
            if (--q >= 0) {
              top = below;
              if (q >= 1) below = load_apex(stk, sg, (size_t)(q - 1) * H);
            }
          }
          if (q < 0) {
            q = 0; top = cand;
            stk[0] = (u32)u; sg[0] = (u16)gu;
          } else if (gu != kInf || top.g2 == (u32)kInf2) {
            // a column without a source never wins over one with a source, and below an apex without a source there are only such
            // apexes, which a column with a source has just popped: here both heights are real or both are kInf^2, and the first
            // column at which u wins, 1 + (u^2 - s^2 + g(u)^2 - g(s)^2) / (2 (u - s)), has a numerator in [0, 2^31)
            const u32 num = (u32)(u * u - top.s * top.s) + gu2 - top.g2;
            const u32 wcol = 1 + num / (u32)(2 * (u - top.s));
            if (wcol < (u32)W) {
              below = top;
              ++q; top = Apex{u, (int)wcol, gu2};
              stk[(size_t)q * H] = (u32)u | (wcol << 16); sg[(size_t)q * H] = (u16)gu;
            }
          }
        }
      }
    }
    for (int c0 = chunks - 1; c0 >= 0; --c0) {
      const int x0 = c0 * kTile, nx = min(kTile, W - x0);
      __syncthreads();
      if (valid) {
        for (int c = nx - 1; c >= 0; --c) {
          const int u = x0 + c;
          const u64 v = height_at(u, top);
          tile[lane][c] = v >= (u64)kInf2 ? kNone : (int)v;
          if (u == top.t && --q >= 0) {
            top = below;
            if (q >= 1) below = load_apex(stk, sg, (size_t)(q - 1) * H);
          }
        }
      }
      __syncthreads();
      for (int rr = 0; rr < kTile; ++rr)
        if (y0 + rr < H && lane < nx) di[(size_t)(y0 + rr) * W + x0 + lane] = tile[rr][lane];
    }
  }
}

// sum over the workgroup in a fixed order: lanes by halving, then the waves one after the other -> valid in thread 0
__device__ __forceinline__ double block_sum_fixed(double v, double* s_w) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kWaves; ++w) t += s_w[w];
  return t;
}
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_down(v, s, 64));
  return v;
}

// maps: D2(dG), D2(dP), D2(P), d2_plane entries apart.  partials: [N][kPixBlocks][2], every workgroup writes its own pair.
__global__ void __launch_bounds__(kThreads) md_gather(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                      const int* __restrict__ maps, size_t d2_plane, const Rec* __restrict__ recs,
                                                      long long* __restrict__ acc, double* __restrict__ partials) {
  __shared__ double s_w[kWaves];
  const Rec r = recs[blockIdx.y];
  const int H = r.h, W = r.w;
  const uint8_t* P = pred + r.off;
  const uint8_t* G = truth + r.off;
  const int* A = maps + r.off;
  const int* B = A + d2_plane;
  const int* Cv = B + d2_plane;
  const long long pixels = (long long)H * W;
  long long np = 0, ng = 0;
  int ma = 0, mb = 0, cover = -1;
  double sa = 0, sb = 0;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < pixels; k += (long long)gridDim.x * kThreads) {
    const int y = (int)(k / W), x = (int)(k % W);
    if (border_at(P, H, W, y, x)) { const int v = A[k]; ++np; ma = max(ma, v); sa += sqrt((double)v); }
    if (G[k] > 127) {
      cover = max(cover, Cv[k]);
      if (border_at(G, H, W, y, x)) { const int v = B[k]; ++ng; mb = max(mb, v); sb += sqrt((double)v); }
    }
  }
  const double ta = block_sum_fixed(sa, s_w), tb = block_sum_fixed(sb, s_w);
  if (threadIdx.x == 0) {
    double* out = partials + ((size_t)blockIdx.y * kPixBlocks + blockIdx.x) * 2;
    out[0] = ta; out[1] = tb;
  }
  if (H == 0) return;
  np = wave_sum(np); ng = wave_sum(ng); ma = wave_max(ma); mb = wave_max(mb); cover = wave_max(cover);
  if ((threadIdx.x & 63) == 0) {
    long long* a = acc + (size_t)blockIdx.y * kAcc;
    if (np) atomicAdd((u64*)a + 0, (u64)np);
    if (ng) atomicAdd((u64*)a + 1, (u64)ng);
    if (ma) atomicMax(a + 2, (long long)ma);
    if (mb) atomicMax(a + 3, (long long)mb);
    if (cover >= 0) atomicMax(a + 4, (long long)cover);
  }
}

// one thread per image: the ranks of the two order statistics, and the sums of the partials in their order
__global__ void __launch_bounds__(kThreads) md_begin(const Rec* __restrict__ recs, const long long* __restrict__ acc, long long* __restrict__ sel,
                                                     const double* __restrict__ partials, int blocks, double* __restrict__ sums, int N) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const long long np = acc[(size_t)i * kAcc], ng = acc[(size_t)i * kAcc + 1];
  const bool active = recs[i].h != 0 && np > 0 && ng > 0;
  double sa = 0, sb = 0;
  if (active)
    for (int b = 0; b < blocks; ++b) { sa += partials[((size_t)i * kPixBlocks + b) * 2]; sb += partials[((size_t)i * kPixBlocks + b) * 2 + 1]; }
  sums[(size_t)i * 2] = sa;
  sums[(size_t)i * 2 + 1] = sb;
  long long* s = sel + (size_t)i * kSel;
  if (active) {
    const long long n = np + ng, lo = 95 * (n - 1) / 100, rem = 95 * (n - 1) % 100;
    s[2] = lo; s[3] = lo + (rem > 0); s[4] = 1; s[5] = rem;
  }
}

// hist[i][k][digit] += the border distances whose bits above shift + 8 equal prefix k, by their eight bits from `shift` on
__global__ void __launch_bounds__(kThreads) md_hist(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                    const int* __restrict__ maps, size_t d2_plane, const Rec* __restrict__ recs,
                                                    const long long* __restrict__ sel, u64* __restrict__ hist, int shift) {
  __shared__ u32 s_h[2][256];
  const Rec r = recs[blockIdx.y];
  const long long* s = sel + (size_t)blockIdx.y * kSel;
  if (r.h == 0 || s[4] == 0) return;
  const int H = r.h, W = r.w;
  const uint8_t* P = pred + r.off;
  const uint8_t* G = truth + r.off;
  const int* A = maps + r.off;
  const int* B = A + d2_plane;
  const u64 p0 = (u64)s[0], p1 = (u64)s[1];
  s_h[0][threadIdx.x] = 0; s_h[1][threadIdx.x] = 0;
  __syncthreads();
  const long long pixels = (long long)H * W;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < pixels; k += (long long)gridDim.x * kThreads) {
    const int y = (int)(k / W), x = (int)(k % W);
    for (int m = 0; m < 2; ++m) {
      if (!border_at(m ? G : P, H, W, y, x)) continue;
      const u64 v = (u64)(u32)(m ? B : A)[k], hi = v >> (shift + 8);
      const int digit = (int)(v >> shift) & 255;
      if (hi == p0) atomicAdd(&s_h[0][digit], 1u);
      if (hi == p1) atomicAdd(&s_h[1][digit], 1u);
    }
  }
  __syncthreads();
  u64* h = hist + (size_t)blockIdx.y * 512;
  for (int k = 0; k < 2; ++k)
    if (s_h[k][threadIdx.x]) atomicAdd(h + k * 256 + threadIdx.x, (u64)s_h[k][threadIdx.x]);
}

// one workgroup per image: the digit in which each rank falls joins its prefix; the last round writes the record
__global__ void __launch_bounds__(kThreads) md_step(const Rec* __restrict__ recs, const long long* __restrict__ acc, long long* __restrict__ sel,
                                                    u64* __restrict__ hist, long long* __restrict__ records, int last) {
  __shared__ long long s_a[kThreads], s_b[kThreads];
  const int i = blockIdx.x, t = threadIdx.x;
  long long* s = sel + (size_t)i * kSel;
  u64* h = hist + (size_t)i * 512;
  const bool active = s[4] != 0;
  const long long ha = (long long)h[t], hb = (long long)h[256 + t];
  const long long ra = s[2], rb = s[3], pa = s[0], pb = s[1];
  s_a[t] = ha; s_b[t] = hb;
  block_scan_incl(s_a, t, s_b);
  const long long ea = s_a[t] - ha, eb = s_b[t] - hb;
  h[t] = 0; h[256 + t] = 0;
  __syncthreads();
  if (active && ea <= ra && ra < s_a[t]) { s[0] = (pa << 8) | t; s[2] = ra - ea; }
  if (active && eb <= rb && rb < s_b[t]) { s[1] = (pb << 8) | t; s[3] = rb - eb; }
  if (!last) return;
  __syncthreads();
  if (t != 0) return;
  long long* out = records + (size_t)i * 10;
  const long long* a = acc + (size_t)i * kAcc;
  for (int j = 0; j < 10; ++j) out[j] = 0;
  if (recs[i].h == 0) { out[9] = 1; return; }
  const long long np = a[0], ng = a[1];
  out[0] = np; out[1] = ng;
  out[7] = ng == 0 ? 0 : np == 0 ? -1 : a[4];
  if (np == 0 && ng == 0) { out[8] = 1; return; }
  if (np == 0 || ng == 0) { out[2] = out[3] = out[4] = out[5] = -1; return; }
  out[2] = a[2]; out[3] = a[3]; out[4] = s[0]; out[5] = s[1]; out[6] = s[5]; out[8] = 1;
}

struct DistLayout {            // workspace: records [, accumulators, select state, histograms, partials], then the planes
  size_t entries, acc, sel, hist, partials, g, stack, sg, d2, total;
};
DistLayout dist_layout(int N, size_t mask_bytes, int surface) {
  DistLayout l;
  const int Z = surface ? 3 : 1;
  l.entries = rup256(mask_bytes);
  size_t at = rup256((size_t)N * sizeof(Rec));
  l.acc = at;      at += surface ? rup256((size_t)N * kAcc * 8) : 0;
  l.sel = at;      at += surface ? rup256((size_t)N * kSel * 8) : 0;
  l.hist = at;     at += surface ? rup256((size_t)N * 512 * 8) : 0;
  l.partials = at; at += surface ? rup256((size_t)N * kPixBlocks * 2 * 8) : 0;
  l.stack = at;    at += (size_t)Z * l.entries * 4;
  l.d2 = at;       at += surface ? (size_t)Z * l.entries * 4 : 0;
  l.g = at;        at += (size_t)Z * l.entries * 2;
  l.sg = at;       at += (size_t)Z * l.entries * 2;
  l.total = at;
  return l;
}

unsigned grid_for(size_t work, size_t per_block, unsigned most) {
  const size_t g = (work + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : g > most ? most : g);
}

// prep, columns, rows of Z transforms
hipError_t launch_transforms(const uint8_t* pred, const uint8_t* truth, int surface, size_t mask_bytes, const ImageDesc* descs, int N,
                             long long max_pixels, long long rows, int* d2, size_t d2_plane, char* ws, const DistLayout& l, hipStream_t st) {
  Rec* recs = (Rec*)ws;
  const unsigned Z = surface ? 3 : 1;
  const size_t side = (size_t)(max_pixels < kMaxSide ? max_pixels : kMaxSide);
  hipLaunchKernelGGL(md_prep, dim3(1), dim3(kThreads), 0, st, descs, recs, surface ? (long long*)(ws + l.acc) : nullptr,
                     surface ? (long long*)(ws + l.sel) : nullptr, surface ? (u64*)(ws + l.hist) : nullptr, N, (long long)mask_bytes, max_pixels,
                     rows, (long long)(mask_bytes / 64 + (size_t)rows));
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(md_columns, dim3(grid_for(side, kThreads, kColBlocks), (unsigned)N, Z), dim3(kThreads), 0, st, pred, truth, surface,
                     (u16*)(ws + l.g), l.entries, recs);
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(md_rows, dim3(grid_for(side, kTile, kRowBlocks), (unsigned)N, Z), dim3(64), 0, st, (const u16*)(ws + l.g),
                     (u32*)(ws + l.stack), (u16*)(ws + l.sg), l.entries, d2, d2_plane, recs);
  return hipGetLastError();
}

}  // namespace

size_t edt_workspace_bytes(int N, size_t mask_bytes, long long) { return dist_layout(N, mask_bytes, 0).total; }
size_t surface_distances_workspace_bytes(int N, size_t mask_bytes, long long) { return dist_layout(N, mask_bytes, 1).total; }

hipError_t launch_edt_ragged(const uint8_t* masks, size_t mask_bytes, const ImageDesc* descs, int N, long long max_pixels, long long rows,
                             int* d2, void* ws, hipStream_t st) {
  const DistLayout l = dist_layout(N, mask_bytes, 0);
  return launch_transforms(masks, masks, 0, mask_bytes, descs, N, max_pixels, rows, d2, 0, (char*)ws, l, st);
}

hipError_t launch_surface_distances_ragged(const uint8_t* pred, const uint8_t* truth, size_t mask_bytes, const ImageDesc* descs, int N,
                                           long long max_pixels, long long rows, long long* records, double* sums, void* wsv, hipStream_t st) {
  char* ws = (char*)wsv;
  const DistLayout l = dist_layout(N, mask_bytes, 1);
  const Rec* recs = (const Rec*)ws;
  long long* acc = (long long*)(ws + l.acc);
  long long* sel = (long long*)(ws + l.sel);
  u64* hist = (u64*)(ws + l.hist);
  double* partials = (double*)(ws + l.partials);
  int* maps = (int*)(ws + l.d2);
  UWM_CHK(launch_transforms(pred, truth, 1, mask_bytes, descs, N, max_pixels, rows, maps, l.entries, ws, l, st));
  // the pixel grids depend on max_pixels alone, so the order of the sums does too
  const dim3 pix(grid_for((size_t)max_pixels, 8 * kThreads, kPixBlocks), (unsigned)N);
  hipLaunchKernelGGL(md_gather, pix, dim3(kThreads), 0, st, pred, truth, (const int*)maps, l.entries, recs, acc, partials);
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(md_begin, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, st, recs, (const long long*)acc, sel,
                     (const double*)partials, (int)pix.x, sums, N);
  UWM_CHK(hipGetLastError());
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(md_hist, pix, dim3(kThreads), 0, st, pred, truth, (const int*)maps, l.entries, recs, (const long long*)sel, hist, shift);
    UWM_CHK(hipGetLastError());
    hipLaunchKernelGGL(md_step, dim3((unsigned)N), dim3(kThreads), 0, st, recs, (const long long*)acc, sel, hist, records, shift == 0);
    UWM_CHK(hipGetLastError());
  }
  return hipSuccess;
}

}  // namespace uwm
