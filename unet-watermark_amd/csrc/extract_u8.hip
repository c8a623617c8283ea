// Watermark cut-outs from watermarked / clean pairs on the device: the reference's extract_watermarks.py for a ragged batch.  The rule
// is stated in include/uwm.h and DESIGN.md 8m.  Integer work throughout, except the Pillow enhancement of stage 2, whose float32
// operations are spelt out one by one (built with -ffp-contract=off): every result is exact and the same on every run.
//
// Stage 1 (extract_regions): difference mask -> close3 -> open3 -> fill -> 8-connected regions -> polygon sums -> kept regions.
// Planes are one byte per pixel.  Both labellings (the 4-connected background for the fill, the 8-connected regions) are one
// union-find with integer atomicMin, the scheme of mask_post.hip restated for byte planes: a label is the pixel's parent, -1 outside
// the set; a parent never exceeds its child, so every walk descends and ends by its own progress, and a finished root is the set's
// first pixel in raster order.  A pixel starts at the head of its run inside its wave's 64 pixels (one ballot), so the chains the
// joins have to walk are short.  No launch waits on another workgroup; there are no propagation rounds.
//
// Every image's working planes lie at a prefix sum of the pixel counts (extract_prep), never at an offset a descriptor names, so
// the labels of one image cannot be reached from another whatever the descriptors hold.  All geometry is read from DEVICE memory;
// grids are sized from the capacities (max_pixels, N; max_crop_pixels, J) alone.
#include "uwm_kernels.h"

namespace uwm {

typedef unsigned long long u64;

namespace {

#include "image_common.inc"

constexpr int kT = 256;
constexpr int kKept = kExtractMaxRegions;        // 254
constexpr int kRow = kExtractRowInts;            // 9
constexpr int kList = 256;                       // ints of one image's list of kept ids

struct XRec {                  // stage 1: one per image, written by extract_prep; h == 0: misfit
  long long wm, clean, plane, ws;
  int h, w;
};
struct XCtr { unsigned found, kept; };

struct XWs {
  XRec* recs;
  XCtr* ctr;
  int* list;
  uint8_t *a, *b;
  int* lab;
  unsigned* acc;
};

struct XLayout { size_t ctr, list, a, b, lab, acc, total; };
XLayout x_layout(int N, long long total_pixels) {
  XLayout l;
  const size_t P = (size_t)total_pixels;
  l.ctr = rup256((size_t)N * sizeof(XRec));
  l.list = l.ctr + rup256((size_t)N * sizeof(XCtr));
  l.a = l.list + rup256((size_t)N * kList * 4);
  l.b = l.a + rup256(P);
  l.lab = l.b + rup256(P);
  l.acc = l.lab + rup256(P * 4);
  l.total = l.acc + rup256(P * 4);
  return l;
}
XWs x_ws(void* ws, const XLayout& l) {
  char* p = (char*)ws;
  return {(XRec*)p, (XCtr*)(p + l.ctr), (int*)(p + l.list), (uint8_t*)(p + l.a), (uint8_t*)(p + l.b), (int*)(p + l.lab), (unsigned*)(p + l.acc)};
}

// one workgroup: validates every pair and lays the working planes out one after the other (prefix sums over N in turns of kT)
__global__ void __launch_bounds__(kT) extract_prep(const ImageDesc* __restrict__ wd, size_t wm_bytes, const ImageDesc* __restrict__ cd,
                                                   size_t clean_bytes, const ImageDesc* __restrict__ pd, size_t plane_bytes, XRec* __restrict__ recs,
                                                   XCtr* __restrict__ ctr, int N, long long max_pixels, long long total_pixels) {
  __shared__ long long s_pix[kT], s_carry;
  const int t = threadIdx.x;
  if (t == 0) s_carry = 0;
  for (int base = 0; base < N; base += kT) {
    __syncthreads();
    const int i = base + t;
    XRec r = {0, 0, 0, 0, 0, 0};
    if (i < N) {
      const ImageDesc w = wd[i], c = cd[i], p = pd[i];
      if (region_ok(w, 3, wm_bytes, 3) && region_ok(c, 3, clean_bytes, 3) && region_ok(p, 1, plane_bytes, 3) && c.h == w.h && c.w == w.w && p.h == w.h &&
          p.w == w.w && (long long)w.h * w.w <= max_pixels) {
        r.wm = w.offset; r.clean = c.offset; r.plane = p.offset; r.h = w.h; r.w = w.w;
      }
      ctr[i].found = 0; ctr[i].kept = 0;
    }
    const long long mine = (long long)r.h * r.w;
    s_pix[t] = mine;
    block_scan_incl(s_pix, t);
    const long long to = s_carry + s_pix[t];
    if (to > total_pixels) r.h = r.w = 0;                    // beyond the capacity: a misfit (it still counts in the sums, as in mask_post.hip)
    r.ws = r.h ? to - mine : 0;
    if (i < N) recs[i] = r;
    __syncthreads();
    if (t == kT - 1) s_carry = to;
  }
}

// m = gray(|wm - clean|) > T: cv2.absdiff -> cvtColor(RGB2GRAY), OpenCV 4.x's 15-bit rule (pair_mask_u8.hip) -> threshold
__global__ void __launch_bounds__(kT) extract_mask(const uint8_t* __restrict__ wm, const uint8_t* __restrict__ clean, const XRec* __restrict__ recs,
                                                   uint8_t* __restrict__ out, int thr) {
  const XRec r = recs[blockIdx.y];
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  if (p >= (unsigned)r.h * r.w) return;
  const uint8_t* a = wm + r.wm + (size_t)p * 3;
  const uint8_t* b = clean + r.clean + (size_t)p * 3;
  const int dr = abs((int)a[0] - (int)b[0]), dg = abs((int)a[1] - (int)b[1]), db = abs((int)a[2] - (int)b[2]);
  const int g = (dr * 9798 + dg * 19235 + db * 3735 + 16384) >> 15;
  out[r.ws + p] = g > thr;
}

// one pass of the 3 x 3 RECT element on a plane of 0 / 1 bytes; pixels outside the image are ignored (0 for the dilation, 1 for the erosion)
template <bool DIL>
__global__ void __launch_bounds__(kT) extract_morph(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const XRec* __restrict__ recs) {
  const XRec r = recs[blockIdx.y];
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  if (p >= (unsigned)r.h * r.w) return;
  const int y = p / r.w, x = p % r.w;
  const uint8_t* s = src + r.ws;
  int v = DIL ? 0 : 1;
  for (int dy = -1; dy <= 1; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= r.h) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= r.w) continue;
      const int q = s[(size_t)yy * r.w + xx];
      v = DIL ? (v | q) : (v & q);
    }
  }
  dst[r.ws + p] = (uint8_t)v;
}

// ---------------------------------------------------------------- union-find on byte planes (image_common.inc's, labels = parent)
// BG: the set is the plane's zeros (the background, for the fill), else its ones.  label = head of the pixel's run inside the wave's
// 64 consecutive pixels (a run also ends where a row does), -1 outside the set; acc = 0
template <bool BG>
__global__ void __launch_bounds__(kT) extract_cc_init(const uint8_t* __restrict__ plane, int* __restrict__ labels, unsigned* __restrict__ acc,
                                                      const XRec* __restrict__ recs) {
  const XRec r = recs[blockIdx.y];
  const unsigned total = (unsigned)r.h * r.w;
  if (blockIdx.x * kT >= total) return;                      // uniform in the workgroup (a misfit has total 0)
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = p < total && (plane[r.ws + p] != 0) != BG;
  const bool row0 = p < total && p % r.w == 0;
  const u64 word = __ballot(in), rows = __ballot(row0);
  const u64 starts = word & ~((word << 1) & ~rows);
  if (p >= total) return;
  int l = -1;
  if (in) {
    const u64 below = starts & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));      // never empty: a run has a head at or below its pixels
    l = (int)p - lane + (63 - __clzll((long long)below));
  }
  labels[r.ws + p] = l;
  acc[r.ws + p] = 0;
}

// joins across wave boundaries and between rows (cc_join)
template <bool CONN8, bool BG>
__global__ void __launch_bounds__(kT) extract_cc_merge(const uint8_t* __restrict__ plane, int* __restrict__ labels, const XRec* __restrict__ recs) {
  const XRec r = recs[blockIdx.y];
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  if (p >= (unsigned)r.h * r.w) return;
  const uint8_t* s = plane + r.ws;
  if ((s[p] != 0) == BG) return;
  const int w = r.w, y = p / w, x = p % w;
  cc_join<CONN8, 0>(labels + r.ws, (int)p, x, y, w, [&](int dy, int dx) { return (s[(int)p + dy * w + dx] != 0) != BG; }, (threadIdx.x & 63) == 0);
}

// labels <- root
__global__ void __launch_bounds__(kT) extract_cc_flatten(int* __restrict__ labels, const XRec* __restrict__ recs) {
  const XRec r = recs[blockIdx.y];
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  if (p >= (unsigned)r.h * r.w) return;
  int* lab = labels + r.ws;
  if (ld_label(lab + p) < 0) return;
  st_label(lab + p, uf_find<0>(lab, (int)p));
}

// acc[root] = 1 for every background component that has a pixel on the image's border: it is 4-connected to the outside
__global__ void __launch_bounds__(kT) extract_border(const int* __restrict__ labels, unsigned* __restrict__ acc, const XRec* __restrict__ recs) {
  const XRec r = recs[blockIdx.y];
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  if (p >= (unsigned)r.h * r.w) return;
  const int y = p / r.w, x = p % r.w;
  if (x != 0 && y != 0 && x != r.w - 1 && y != r.h - 1) return;
  const int l = labels[r.ws + p];
  if (l >= 0) acc[r.ws + l] = 1u;
}

// F = m plus the background that does not reach the outside
__global__ void __launch_bounds__(kT) extract_fill(const uint8_t* __restrict__ m, const int* __restrict__ labels, const unsigned* __restrict__ acc,
                                                   uint8_t* __restrict__ F, const XRec* __restrict__ recs) {
  const XRec r = recs[blockIdx.y];
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  if (p >= (unsigned)r.h * r.w) return;
  const int l = labels[r.ws + p];
  F[r.ws + p] = m[r.ws + p] != 0 || (l >= 0 && acc[r.ws + l] == 0u);
}

// the 2 x 2 window whose bottom-right corner is pixel (x, y), x, y >= 1: the root its corners share and how many are in F.
// Any three corners of a window are 8-neighbours of each other, so three or four in F lie in one region.  (A window that reaches
// outside the image has at most two corners in F and adds nothing.)
__device__ __forceinline__ int window(const int* __restrict__ lab, unsigned p, int w, int& root, int& missing) {
  const int l[4] = {lab[p - w - 1], lab[p - w], lab[p - 1], lab[p]};
  int n = 0;
  root = -1; missing = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (l[k] >= 0) { ++n; root = l[k]; } else missing = k;
  }
  return n;
}

// acc[root] += a00 of the region's windows (2 for four corners, 1 for three).  A wave adds the lanes that share the root of its
// first contributing lane with one atomic
__global__ void __launch_bounds__(kT) extract_a00(const int* __restrict__ labels, unsigned* __restrict__ acc, const XRec* __restrict__ recs) {
  const XRec r = recs[blockIdx.y];
  const unsigned total = (unsigned)r.h * r.w;
  if (blockIdx.x * kT >= total) return;                      // uniform in the workgroup
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  int root = -1, c = 0;
  if (p < total) {
    const int y = p / r.w, x = p % r.w;
    if (x >= 1 && y >= 1) {
      int missing;
      const int n = window(labels + r.ws, p, r.w, root, missing);
      c = n == 4 ? 2 : n == 3 ? 1 : 0;
      if (!c) root = -1;
    }
  }
  const u64 active = __ballot(root >= 0);
  if (!active) return;                                       // uniform in the wave
  const int first = __ffsll((long long)active) - 1;
  const int r0 = __shfl(root, first);
  const bool same = root == r0;
  const unsigned sum = __popcll(__ballot(same && c == 1)) + 2u * __popcll(__ballot(same && c == 2));
  if ((int)(threadIdx.x & 63) == first) atomicAdd(acc + r.ws + r0, sum);
  else if (root >= 0 && !same) atomicAdd(acc + r.ws + root, (unsigned)c);
}

// roots: counted, and those with a00 > 2 * min_area (contourArea > min_area) appended to the image's list, in any order
__global__ void __launch_bounds__(kT) extract_select(const int* __restrict__ labels, const unsigned* __restrict__ acc, XCtr* __restrict__ ctr,
                                                     int* __restrict__ list, const XRec* __restrict__ recs, long long min2) {
  const XRec r = recs[blockIdx.y];
  const unsigned total = (unsigned)r.h * r.w;
  if (blockIdx.x * kT >= total) return;
  const unsigned p = blockIdx.x * kT + threadIdx.x;
  const bool is_root = p < total && labels[r.ws + p] == (int)p;
  const u64 roots = __ballot(is_root);
  if (!roots) return;
  if ((int)(threadIdx.x & 63) == __ffsll((long long)roots) - 1) atomicAdd(&ctr[blockIdx.y].found, (unsigned)__popcll(roots));
  if (is_root && (long long)acc[r.ws + p] > min2) {
    const unsigned slot = atomicAdd(&ctr[blockIdx.y].kept, 1u);
    if (slot < (unsigned)kKept) list[(size_t)blockIdx.y * kList + slot] = (int)p;
  }
}

// one workgroup per image: the list in ascending id order (ids differ: rank = the number of smaller ones), the table rows
// initialised, the image's stats written.  More than kKept kept regions: status 2, an empty table
__global__ void __launch_bounds__(kT) extract_sort(const XRec* __restrict__ recs, XCtr* __restrict__ ctr, int* __restrict__ list,
                                                   long long* __restrict__ stats, long long* __restrict__ table) {
  __shared__ int s_id[kList];
  const int n = blockIdx.x, t = threadIdx.x;
  const XRec r = recs[n];
  const unsigned found = ctr[n].found, kept = ctr[n].kept;
  const int status = r.h == 0 ? 1 : kept > (unsigned)kKept ? 2 : 0;
  const int k = status == 0 ? (int)kept : 0;
  int* mine = list + (size_t)n * kList;
  if (t < k) s_id[t] = mine[t];
  __syncthreads();
  int rank = 0, id = 0;
  if (t < k) {
    id = s_id[t];
    for (int j = 0; j < k; ++j) rank += s_id[j] < id;
  }
  __syncthreads();
  if (t < k) mine[rank] = id;
  else if (t < kList) mine[t] = 0x7fffffff;
  long long* rows = table + (size_t)n * kKept * kRow;
  for (int i = t; i < kKept * kRow; i += kT) rows[i] = 0;
  __syncthreads();
  if (t < k) {
    long long* row = rows + (size_t)rank * kRow;
    row[0] = id;
    row[4] = 1ll << 40; row[5] = 1ll << 40;                  // x0, y0: minima
  }
  if (t == 0) {
    long long* s = stats + (size_t)n * 4;
    s[0] = status == 1 ? 0 : found;
    s[1] = status == 1 ? 0 : kept;
    s[2] = status;
    s[3] = (long long)r.h * r.w;
  }
}

// index of `root` in the ascending list of k ids, or 255
__device__ __forceinline__ int kept_index(const int* s_id, int k, int root) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_id[mid] < root) lo = mid + 1; else hi = mid;
  }
  return lo < k && s_id[lo] == root ? lo : 255;
}

// the plane (index of the kept region at each pixel, 255 for none) and the kept regions' sums: per workgroup in LDS, then one
// global atomic per touched entry.  Integer sums and extrema: any order, one result
__global__ void __launch_bounds__(kT) extract_sums(const int* __restrict__ labels, const XRec* __restrict__ recs, const XCtr* __restrict__ ctr,
                                                   const int* __restrict__ list, uint8_t* __restrict__ plane, long long* __restrict__ table) {
  __shared__ int s_id[kList];
  __shared__ u64 s_sum[kKept][3];
  __shared__ int s_box[kKept][4];
  __shared__ unsigned s_pix[kKept];
  const XRec r = recs[blockIdx.y];
  const unsigned total = (unsigned)r.h * r.w;
  if (blockIdx.x * kT >= total) return;                      // uniform in the workgroup
  const unsigned kept = ctr[blockIdx.y].kept;
  const int k = kept > (unsigned)kKept ? 0 : (int)kept;
  const int t = threadIdx.x;
  if (t < k) {
    s_id[t] = list[(size_t)blockIdx.y * kList + t];
    s_sum[t][0] = s_sum[t][1] = s_sum[t][2] = 0;
    s_box[t][0] = s_box[t][1] = 0x7fffffff; s_box[t][2] = s_box[t][3] = -1;
    s_pix[t] = 0;
  }
  __syncthreads();
  const unsigned p = blockIdx.x * kT + t;
  if (p < total) {
    const int* lab = labels + r.ws;
    const int y = p / r.w, x = p % r.w;
    const int l = lab[p];
    const int idx = l >= 0 ? kept_index(s_id, k, l) : 255;
    plane[r.plane + p] = (uint8_t)idx;
    if (idx != 255) {
      atomicAdd(&s_pix[idx], 1u);
      atomicMin(&s_box[idx][0], x); atomicMin(&s_box[idx][1], y);
      atomicMax(&s_box[idx][2], x); atomicMax(&s_box[idx][3], y);
    }
    if (k && x >= 1 && y >= 1) {
      int root, missing;
      const int n = window(lab, p, r.w, root, missing);
      if (n >= 3) {
        const int wi = root == l ? idx : kept_index(s_id, k, root);
        if (wi != 255) {
          u64 a00, a10, a01;
          if (n == 4) { a00 = 2; a10 = 6ull * (x - 1) + 3; a01 = 6ull * (y - 1) + 3; }
          else {                                             // the three corners' coordinates: all four, less the missing one
            a00 = 1;
            a10 = 4ull * x - 2 - (u64)(x - 1 + (missing & 1));
            a01 = 4ull * y - 2 - (u64)(y - 1 + (missing >> 1));
          }
          atomicAdd(&s_sum[wi][0], a00); atomicAdd(&s_sum[wi][1], a10); atomicAdd(&s_sum[wi][2], a01);
        }
      }
    }
  }
  __syncthreads();
  if (t < k && (s_pix[t] != 0 || s_sum[t][0] != 0)) {
    u64* row = (u64*)(table + ((size_t)blockIdx.y * kKept + t) * kRow);      // (every entry is non-negative)
    if (s_sum[t][0]) { atomicAdd(row + 1, s_sum[t][0]); atomicAdd(row + 2, s_sum[t][1]); atomicAdd(row + 3, s_sum[t][2]); }
    if (s_pix[t]) {
      atomicMin(row + 4, (u64)s_box[t][0]); atomicMin(row + 5, (u64)s_box[t][1]);
      atomicMax(row + 6, (u64)s_box[t][2]); atomicMax(row + 7, (u64)s_box[t][3]);
      atomicAdd(row + 8, (u64)s_pix[t]);
    }
  }
}

// ---------------------------------------------------------------- stage 2: cut-outs
struct CRec { long long wm, plane; int W, ok; };            // one per job, written by cutout_prep
struct CLayout { size_t sums, total; };
CLayout c_layout(int J) {
  CLayout l;
  l.sums = rup256((size_t)J * sizeof(CRec));
  l.total = l.sums + rup256((size_t)J * 8);
  return l;
}

__global__ void __launch_bounds__(kT) cutout_prep(const ImageDesc* __restrict__ wd, size_t wm_bytes, const ImageDesc* __restrict__ pd, size_t plane_bytes,
                                                  int N, const ExtractJob* __restrict__ jobs, int J, long long max_crop_pixels, size_t out_bytes,
                                                  CRec* __restrict__ recs, u64* __restrict__ sums, int* __restrict__ status) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= J) return;
  CRec c = {0, 0, 0, 0};
  const int image = jobs[j].image, x = jobs[j].x, y = jobs[j].y, w = jobs[j].w, h = jobs[j].h;
  const long long off = jobs[j].out_offset;
  if (image >= 0 && image < N) {
    const ImageDesc a = wd[image], b = pd[image];
    if (region_ok(a, 3, wm_bytes, 3) && region_ok(b, 1, plane_bytes, 3) && a.h == b.h && a.w == b.w && x >= 0 && y >= 0 && w >= 3 && h >= 3 &&
        (long long)x + w <= a.w && (long long)y + h <= a.h && (long long)w * h <= max_crop_pixels && off >= 0 && (off & 3) == 0 &&
        (u64)off <= out_bytes && (u64)w * (u64)h <= (out_bytes - (u64)off) / 4) {
      c.wm = a.offset; c.plane = b.offset; c.W = a.w; c.ok = 1;
    }
  }
  recs[j] = c;
  sums[j] = 0;
  status[j] = c.ok ? 0 : 1;
}

// sums[j] = the sum of L over the crop (the Contrast degenerate is its rounded mean); integer: any order, one result
__global__ void __launch_bounds__(kT) cutout_luma(const uint8_t* __restrict__ wm, const ExtractJob* __restrict__ jobs, const CRec* __restrict__ recs,
                                                  u64* __restrict__ sums) {
  __shared__ unsigned red[kT];
  const CRec c = recs[blockIdx.y];
  if (!c.ok) return;
  const ExtractJob* jb = jobs + blockIdx.y;
  const int w = jb->w;
  const unsigned total = (unsigned)w * jb->h;
  if (blockIdx.x * kT >= total) return;                      // uniform in the workgroup
  const unsigned i = blockIdx.x * kT + threadIdx.x;
  unsigned v = 0;
  if (i < total) {
    const int cy = i / w, cx = i % w;
    const uint8_t* px = wm + c.wm + ((size_t)(jb->y + cy) * c.W + jb->x + cx) * 3;
    v = luma8(px[0], px[1], px[2]);
  }
  red[threadIdx.x] = v;
  __syncthreads();
  for (int st = kT / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(sums + blockIdx.y, (u64)red[0]);
}

// RGBA of the crop through ImageEnhance.Contrast(1.3), Sharpness(1.4), Brightness(1.1); alpha = 255 on the job's member regions.
// The SMOOTH degenerate of a pixel needs the contrast stage of its eight neighbours, which is recomputed from the image (a blend each)
__global__ void __launch_bounds__(kT) cutout_final(const uint8_t* __restrict__ wm, const uint8_t* __restrict__ plane, const ExtractJob* __restrict__ jobs,
                                                   const CRec* __restrict__ recs, const u64* __restrict__ sums, uint8_t* __restrict__ out) {
  const CRec c = recs[blockIdx.y];
  if (!c.ok) return;
  const ExtractJob* jb = jobs + blockIdx.y;
  const int w = jb->w, h = jb->h;
  const unsigned total = (unsigned)w * h;
  const unsigned i = blockIdx.x * kT + threadIdx.x;
  if (i >= total) return;
  const int mean = (int)__dadd_rn((double)sums[blockIdx.y] / (double)total, 0.5);
  const float fc = 1.3f, fs = 1.4f, fb = 1.1f;
  const float k1 = __fdiv_rn(1.f, 13.f), k5 = __fdiv_rn(5.f, 13.f);       // ImageFilter.SMOOTH: (1,1,1,1,5,1,1,1,1) / 13 as float32
  const int cy = i / w, cx = i % w;
  const uint8_t* base = wm + c.wm + ((size_t)jb->y * c.W + jb->x) * 3;
  const uint8_t* px = base + ((size_t)cy * c.W + cx) * 3;
  const int idx = plane[c.plane + (size_t)(jb->y + cy) * c.W + jb->x + cx];
  const int alpha = idx != 255 && jb->member[idx] ? 255 : 0;
  const bool inner = cx >= 1 && cy >= 1 && cx < w - 1 && cy < h - 1;      // the one-pixel frame is copied unfiltered
  uint32_t rgba = (uint32_t)alpha << 24;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int v = blend8(mean, px[ch], fc);
    int d = v;
    if (inner) {
      float ss = 0.5f;                                       // Pillow's ImagingFilter3x3: offset + 0.5, then the rows y + 1, y, y - 1
#pragma unroll
      for (int dy = 1; dy >= -1; --dy) {
        const uint8_t* row = px + (ptrdiff_t)dy * c.W * 3 + ch;
        const float a = (float)blend8(mean, row[-3], fc), b = (float)blend8(mean, row[0], fc), e = (float)blend8(mean, row[3], fc);
        const float kc = dy == 0 ? k5 : k1;
        ss = __fadd_rn(ss, __fadd_rn(__fadd_rn(__fmul_rn(a, k1), __fmul_rn(b, kc)), __fmul_rn(e, k1)));
      }
      d = ss <= 0.f ? 0 : ss >= 255.f ? 255 : (int)ss;
    }
    const int s = blend8(d, v, fs);
    rgba |= (uint32_t)blend8(0, s, fb) << (8 * ch);
  }
  *(uint32_t*)(out + jb->out_offset + (size_t)i * 4) = rgba;
}

}  // namespace

size_t extract_workspace_bytes(int N, long long total_pixels, int J) {
  const size_t a = N >= 1 && total_pixels >= 1 ? x_layout(N, total_pixels).total : 0;
  const size_t b = J >= 1 ? c_layout(J).total : 0;
  return a > b ? a : b;
}

hipError_t launch_extract_regions(const uint8_t* wm, size_t wm_bytes, const ImageDesc* wm_descs, const uint8_t* clean, size_t clean_bytes,
                                  const ImageDesc* clean_descs, int N, int threshold, int min_area, long long max_pixels, long long total_pixels,
                                  uint8_t* plane, size_t plane_bytes, const ImageDesc* plane_descs, long long* stats, long long* table, void* ws,
                                  hipStream_t st) {
  const XWs x = x_ws(ws, x_layout(N, total_pixels));
  const dim3 grid((unsigned)((max_pixels + kT - 1) / kT), (unsigned)N), block(kT);
  hipLaunchKernelGGL(extract_prep, dim3(1), block, 0, st, wm_descs, wm_bytes, clean_descs, clean_bytes, plane_descs, plane_bytes, x.recs, x.ctr, N,
                     max_pixels, total_pixels);
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(extract_mask, grid, block, 0, st, wm, clean, x.recs, x.a, threshold);
  hipLaunchKernelGGL(extract_morph<true>, grid, block, 0, st, x.a, x.b, x.recs);       // close
  hipLaunchKernelGGL(extract_morph<false>, grid, block, 0, st, x.b, x.a, x.recs);
  hipLaunchKernelGGL(extract_morph<false>, grid, block, 0, st, x.a, x.b, x.recs);      // open
  hipLaunchKernelGGL(extract_morph<true>, grid, block, 0, st, x.b, x.a, x.recs);
  UWM_CHK(hipGetLastError());
  // the fill: the 4-connected components of the background, those that touch the border marked
  hipLaunchKernelGGL(extract_cc_init<true>, grid, block, 0, st, x.a, x.lab, x.acc, x.recs);
  hipLaunchKernelGGL((extract_cc_merge<false, true>), grid, block, 0, st, x.a, x.lab, x.recs);
  hipLaunchKernelGGL(extract_cc_flatten, grid, block, 0, st, x.lab, x.recs);
  hipLaunchKernelGGL(extract_border, grid, block, 0, st, x.lab, x.acc, x.recs);
  hipLaunchKernelGGL(extract_fill, grid, block, 0, st, x.a, x.lab, x.acc, x.b, x.recs);
  UWM_CHK(hipGetLastError());
  // the regions: the 8-connected components of F
  hipLaunchKernelGGL(extract_cc_init<false>, grid, block, 0, st, x.b, x.lab, x.acc, x.recs);
  hipLaunchKernelGGL((extract_cc_merge<true, false>), grid, block, 0, st, x.b, x.lab, x.recs);
  hipLaunchKernelGGL(extract_cc_flatten, grid, block, 0, st, x.lab, x.recs);
  hipLaunchKernelGGL(extract_a00, grid, block, 0, st, x.lab, x.acc, x.recs);
  hipLaunchKernelGGL(extract_select, grid, block, 0, st, x.lab, x.acc, x.ctr, x.list, x.recs, 2ll * min_area);
  hipLaunchKernelGGL(extract_sort, dim3((unsigned)N), block, 0, st, x.recs, x.ctr, x.list, stats, table);
  hipLaunchKernelGGL(extract_sums, grid, block, 0, st, x.lab, x.recs, x.ctr, x.list, plane, table);
  return hipGetLastError();
}

hipError_t launch_extract_cutouts(const uint8_t* wm, size_t wm_bytes, const ImageDesc* wm_descs, const uint8_t* plane, size_t plane_bytes,
                                  const ImageDesc* plane_descs, int N, const ExtractJob* jobs, int J, long long max_crop_pixels, uint8_t* out,
                                  size_t out_bytes, int* status, void* ws, hipStream_t st) {
  const CLayout l = c_layout(J);
  CRec* recs = (CRec*)ws;
  u64* sums = (u64*)((char*)ws + l.sums);
  const dim3 grid((unsigned)((max_crop_pixels + kT - 1) / kT), (unsigned)J), block(kT);
  hipLaunchKernelGGL(cutout_prep, dim3((unsigned)((J + kT - 1) / kT)), block, 0, st, wm_descs, wm_bytes, plane_descs, plane_bytes, N, jobs, J,
                     max_crop_pixels, out_bytes, recs, sums, status);
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(cutout_luma, grid, block, 0, st, wm, jobs, recs, sums);
  hipLaunchKernelGGL(cutout_final, grid, block, 0, st, wm, plane, jobs, recs, sums, out);
  return hipGetLastError();
}

}  // namespace uwm
