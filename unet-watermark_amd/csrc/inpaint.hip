// Membrane (harmonic) fill of the hole pixels of a ragged batch of images: pull-push as the initial guess, then V-cycles of a
// geometric multigrid on the hole.  DESIGN.md §8v and include/uwm.h are the specification; tests/inpaint_ref.py is the numpy form
// the result is held to byte for byte.  Every float operation is rounded on its own (no contraction), divisions are IEEE.
//
// Layout.  Level 0 of an image is the image, level l + 1 has ceil(h_l / 2) x ceil(w_l / 2) cells.  One flag per cell says "unknown"
// (H_l: all pixels below the cell are hole pixels; the same set is the non-valid cells of the pull), one flag per 32 x 32 tile and
// level says "holds an unknown".  Values are planar per channel.  A cell that is not unknown has a FIXED value that is never stored
// in the iterate: the image byte (level 0), the pulled average v_l (push), zero (V-cycle corrections); so only unknown cells are
// ever written and a tile without one is skipped by every launch after the pull.
//
// Launches.  Levels whose sides fit 64 (all levels from `lc` on, lc from max_side) run in LDS, one workgroup per (image, channel):
// ip_coarse does the push of all of them, or one whole V(lc), in one launch.  The levels below lc run as 32 x 32 tiles with a
// 5-cell halo (ip_tile): a launch loads the tile, runs its two sweeps (four half-sweeps) in LDS and, on the way down, forms the
// residual and restricts it; on the way up it adds the prolonged correction first.  A red-black half-sweep reads only cells of the
// other colour, so ring k of the loaded region is exact after k half-sweeps whatever the neighbours do: the 32 x 32 interior (ring
// >= 5) is exact after four, and so is its residual.  A launch reads one buffer and writes the other (A / B per level), so no
// workgroup reads what another writes in the same launch.  Integer atomics only: results are the same on every run.
//
//   prep, count (hole pixels + level-0 tile flags), status                                             3
//   pull l -> l + 1, l = 0 .. L - 1 (values, cell flags, tile flags, the mask of levels with unknowns)  L
//   push: ip_coarse, then ip_tile<PUSH> l = lc - 1 .. 0                                                 1 + lc
//   per cycle: ip_tile<PRE> l = 0 .. lc - 1, ip_coarse, ip_tile<POST> l = lc - 1 .. 0                   2 lc + 1
//   store                                                                                               1
// with L = ceil(log2(max_side)): the count follows the capacities and `cycles` alone.
#include "uwm_kernels.h"

namespace uwm {

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

#include "image_common.inc"

constexpr int kThreads = 256;
constexpr int kT = 32;                         // tile side (even: a tile's coarse cells are its own)
constexpr int kR = 5;                          // halo: four half-sweeps + the residual
constexpr int kS = kT + 2 * kR;                // 42: side of the loaded region
constexpr int kLds = 64;                       // a level with both sides <= kLds runs in LDS, with every level above it
constexpr int kLdsCells = 5472;                // 64^2 + 32^2 + ... + 1 = 5461 cells at most
enum { PUSH = 0, PRE = 1, POST = 2 };

struct Rec {                   // one per image, written by ip_prep; status as in stats (3: misfit)
  long long ioff, moff;        // bytes into images / out, into masks
  long long base0, basec, baset;   // cells into a level-0 plane, into a coarse plane (levels >= 1), into the tile flags
  int h, w, status, L;
};
struct Ws {
  Rec* recs;
  u64* cnt;                    // [N] hole pixels
  unsigned* lmask;             // [N] bit l: level l holds an unknown
  float *u0a, *u0b;            // [C][p0] level 0 iterate, buffers A and B
  float *ea, *eb, *bc;         // [C][pc] levels >= 1: iterate A, B; right-hand side (during pull and push: the pulled v)
  uint8_t* fc;                 // [pc] levels >= 1: 1 = unknown
  uint8_t* tf;                 // [tc] per tile and level: 1 = holds an unknown
  long long p0, pc, tc;
};
struct Lev { int h, w; long long off, toff; };

__host__ __device__ inline long long tiles_of(int h, int w) { return (long long)((h + kT - 1) / kT) * ((w + kT - 1) / kT); }

__device__ __forceinline__ Lev level_of(const Rec& r, int l) {
  int h = r.h, w = r.w;
  long long coff = r.basec, toff = r.baset;
  for (int k = 0; k < l; ++k) {
    toff += tiles_of(h, w);
    if (k >= 1) coff += (long long)h * w;
    h = (h + 1) >> 1; w = (w + 1) >> 1;
  }
  Lev v; v.h = h; v.w = w; v.off = l == 0 ? r.base0 : coff; v.toff = toff;
  return v;
}

// ---------------------------------------------------------------- prep
// One workgroup: validates every descriptor pair and gives each image its place in the planes (prefix sums over N in turns of 256).
// An image is a misfit when a descriptor does not fit its buffer or the capacities, when the mask's size differs, or when the sums
// up to and including it leave a plane or `rows`
__global__ void __launch_bounds__(kThreads) ip_prep(const ImageDesc* __restrict__ idescs, const ImageDesc* __restrict__ mdescs, Ws ws, int N, int C,
                                                    long long image_bytes, long long mask_bytes, long long max_pixels, long long rows, int max_side,
                                                    long long* __restrict__ stats) {
  __shared__ long long s_px[kThreads], s_cc[kThreads], s_tl[kThreads], s_rw[kThreads];
  __shared__ long long s_carry[4];
  const int t = threadIdx.x;
  if (t < 4) s_carry[t] = 0;
  __syncthreads();
  for (int base = 0; base < N; base += kThreads) {
    const int i = base + t;
    ImageDesc d = {0, 0, 0}, m = {0, 0, 0};
    bool ok = false;
    long long px = 0, cc = 0, tl = 0;
    int L = 0;
    if (i < N) {
      d = idescs[i]; m = mdescs[i];
      ok = region_ok(d, C, (size_t)image_bytes, 1, max_side) && (long long)d.h * d.w <= max_pixels && m.h == d.h && m.w == d.w &&
           region_ok(m, 1, (size_t)mask_bytes, 1, max_side);
      if (ok) {
        const int side = d.h > d.w ? d.h : d.w;
        while ((1 << L) < side) ++L;
        int h = d.h, w = d.w;
        px = (long long)h * w;
        for (int l = 0; l <= L; ++l) {
          tl += tiles_of(h, w);
          if (l >= 1) cc += (long long)h * w;
          h = (h + 1) >> 1; w = (w + 1) >> 1;
        }
      }
    }
    s_px[t] = px; s_cc[t] = cc; s_tl[t] = tl; s_rw[t] = ok ? d.h : 0;
    block_scan_incl(s_px, t, s_cc);
    block_scan_incl(s_tl, t, s_rw);
    const long long epx = s_carry[0] + s_px[t], ecc = s_carry[1] + s_cc[t], etl = s_carry[2] + s_tl[t], erw = s_carry[3] + s_rw[t];
    if (ok && (epx > ws.p0 || ecc > ws.pc || etl > ws.tc || erw > rows)) ok = false;
    if (i < N) {
      Rec r;
      r.ioff = ok ? d.offset : 0; r.moff = ok ? m.offset : 0;
      r.base0 = epx - px; r.basec = ecc - cc; r.baset = etl - tl;
      r.h = ok ? d.h : 0; r.w = ok ? d.w : 0; r.status = ok ? 0 : 3; r.L = L;
      ws.recs[i] = r;
      ws.cnt[i] = 0;
      ws.lmask[i] = 0;
      if (stats) { long long* s = stats + (size_t)i * 4; s[0] = 0; s[1] = ok ? 0 : 3; s[2] = 0; s[3] = 0; }
    }
    __syncthreads();
    if (t == kThreads - 1) { s_carry[0] += s_px[t]; s_carry[1] += s_cc[t]; s_carry[2] += s_tl[t]; s_carry[3] += s_rw[t]; }
    __syncthreads();
  }
}

// hole pixels of every image (integer sum) and the level-0 tile flags; one workgroup per tile, four pixels a thread
__global__ void __launch_bounds__(kThreads) ip_count(const uint8_t* __restrict__ masks, Ws ws) {
  __shared__ unsigned s_cnt[kThreads / 64];
  const Rec rc = ws.recs[blockIdx.y];
  if (rc.status == 3) return;
  const int tw = (rc.w + kT - 1) / kT;
  const long long nt = tiles_of(rc.h, rc.w);
  const uint8_t* mk = masks + rc.moff;
  for (long long tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const int y0 = (int)(tile / tw) * kT, x0 = (int)(tile % tw) * kT;
    unsigned cnt = 0;
    for (int k = threadIdx.x; k < kT * kT; k += kThreads) {
      const int y = y0 + k / kT, x = x0 + k % kT;
      if (y < rc.h && x < rc.w) cnt += mk[(long long)y * rc.w + x] != 0;
    }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned sum = 0;
      for (int k = 0; k < kThreads / 64; ++k) sum += s_cnt[k];
      ws.tf[rc.baset + tile] = sum != 0;
      if (sum) atomicAdd(ws.cnt + blockIdx.y, (u64)sum);
    }
  }
}

// status 1: no hole pixel, 2: no known pixel; both launch nothing more than the copy of ip_store
__global__ void __launch_bounds__(kThreads) ip_status(Ws ws, int N, long long* __restrict__ stats) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  Rec* r = ws.recs + i;
  if (r->status == 3) return;
  const long long holes = (long long)ws.cnt[i], area = (long long)r->h * r->w;
  const int st = holes == 0 ? 1 : holes == area ? 2 : 0;
  r->status = st;
  if (st == 0) ws.lmask[i] = 1;
  if (stats) { stats[(size_t)i * 4] = holes; stats[(size_t)i * 4 + 1] = st; }
}

// ---------------------------------------------------------------- pull: level l -> l + 1
// v = the valid children's sum, in children order, over their number; a cell without a valid child is unknown.  v goes to the
// right-hand-side plane (free until the first V-cycle).  One workgroup per 32 x 32 tile of level l + 1, four cells a thread
__global__ void __launch_bounds__(kThreads) ip_pull(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks, Ws ws, int l, int C) {
  const Rec rc = ws.recs[blockIdx.y];
  if (rc.status != 0 || l >= rc.L) return;
  const Lev f = level_of(rc, l), c = level_of(rc, l + 1);
  const int tw = (c.w + kT - 1) / kT;
  const long long nt = tiles_of(c.h, c.w);
  const uint8_t* img = images + rc.ioff;
  const uint8_t* mk = masks + rc.moff;
  bool any_wg = false;
  for (long long tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    const int y0 = (int)(tile / tw) * kT, x0 = (int)(tile % tw) * kT;
    int any = 0;
    for (int k = threadIdx.x; k < kT * kT; k += kThreads) {
      const int Y = y0 + k / kT, X = x0 + k % kT;
      if (Y >= c.h || X >= c.w) continue;
      long long ci[4];
      int n = 0;
      for (int j = 0; j < 4; ++j) {
        const int y = 2 * Y + (j >> 1), x = 2 * X + (j & 1);
        if (y >= f.h || x >= f.w) continue;
        const long long p = (long long)y * f.w + x;
        const bool unknown = l == 0 ? mk[p] != 0 : ws.fc[f.off + p] != 0;
        if (!unknown) ci[n++] = p;
      }
      const long long P = c.off + (long long)Y * c.w + X;
      ws.fc[P] = n == 0;
      any |= n == 0;
      for (int ch = 0; ch < C; ++ch) {
        float s = 0.f;
        for (int j = 0; j < n; ++j) {
          const float v = l == 0 ? (float)img[ci[j] * C + ch] : ws.bc[ch * ws.pc + f.off + ci[j]];
          s = j == 0 ? v : s + v;
        }
        ws.bc[ch * ws.pc + P] = n ? __fdiv_rn(s, (float)n) : 0.f;
      }
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) ws.tf[c.toff + tile] = any != 0;
    any_wg |= any != 0;
  }
  if (threadIdx.x == 0 && any_wg) atomicOr(ws.lmask + blockIdx.y, 1u << (l + 1));
}

// ---------------------------------------------------------------- shared arithmetic
// the value of a cell of level l + 1 as the prolongation sees it: the iterate where unknown, else the fixed value
template <int MODE>
__device__ __forceinline__ float coarse_at(const Ws& ws, const float* __restrict__ src, const Lev& c, int ch, int y, int x) {
  const long long p = c.off + (long long)y * c.w + x;
  if (ws.fc[p]) return src[ch * ws.pc + p];
  return MODE == PUSH ? ws.bc[ch * ws.pc + p] : 0.f;
}
__device__ __forceinline__ float up4(float a, float b, float c, float d) { return ((9.f * a + 3.f * b) + (3.f * c + d)) * 0.0625f; }
__device__ __forceinline__ int other(int p, int y, int n) { return min(max(p + ((y & 1) ? 1 : -1), 0), n - 1); }

// one half-sweep over a region of LDS: cells of colour `col` (global parity) that are unknown get (b + S) / cnt.  v / b / fl are the
// region's planes of row pitch `pitch`; (gy0, gx0) its origin in the level h x w; rows / columns [lo, hi) of the region are updated
__device__ __forceinline__ void half_sweep(float* v, const float* b, const uint8_t* fl, int pitch, int lo, int hi_y, int hi_x, int gy0, int gx0,
                                           int h, int w, int col) {
  const int ny = hi_y - lo, nx = hi_x - lo;
  for (int k = threadIdx.x; k < ny * nx; k += kThreads) {
    const int ry = lo + k / nx, rx = lo + k % nx;
    const int gy = gy0 + ry, gx = gx0 + rx;
    const int i = ry * pitch + rx;
    if (fl[i] != 1 || ((gy + gx) & 1) != col) continue;
    float s = 0.f;
    int cnt = 0;
    if (gy > 0) { s = v[i - pitch]; cnt = 1; }
    if (gx > 0) { s = cnt ? s + v[i - 1] : v[i - 1]; ++cnt; }
    if (gx + 1 < w) { s = cnt ? s + v[i + 1] : v[i + 1]; ++cnt; }
    if (gy + 1 < h) { s = cnt ? s + v[i + pitch] : v[i + pitch]; ++cnt; }
    if (cnt) v[i] = __fdiv_rn(b[i] + s, (float)cnt);
  }
}
// r = b - (cnt * u - S) of an unknown cell
__device__ __forceinline__ float residual_at(const float* v, const float* b, int pitch, int i, int gy, int gx, int h, int w) {
  float s = 0.f;
  int cnt = 0;
  if (gy > 0) { s = v[i - pitch]; cnt = 1; }
  if (gx > 0) { s = cnt ? s + v[i - 1] : v[i - 1]; ++cnt; }
  if (gx + 1 < w) { s = cnt ? s + v[i + 1] : v[i + 1]; ++cnt; }
  if (gy + 1 < h) { s = cnt ? s + v[i + pitch] : v[i + pitch]; ++cnt; }
  return b[i] - ((float)cnt * v[i] - s);
}

// ---------------------------------------------------------------- the levels below lc: tiles with a halo
// MODE PUSH: u = up(g_{l+1}) on the unknowns, one sweep with b = 0, fixed values v_l; -> buffer A
//      PRE : two sweeps from buffer A (level 0) or from zero (levels >= 1), then b_{l+1} = the restricted residual; -> B (0) / A (>= 1)
//      POST: u += up(e_{l+1}), two sweeps; B -> A (level 0), A -> B (levels >= 1).  e_{l+1} is read from buffer B of level l + 1
template <int MODE>
__global__ void __launch_bounds__(kThreads) ip_tile(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks, Ws ws, int l, int C) {
  __shared__ float s_v[kS * kS], s_b[kS * kS], s_r[kT * kT];
  __shared__ uint8_t s_f[kS * kS];
  const Rec rc = ws.recs[blockIdx.y];
  if (rc.status != 0 || l >= rc.L) return;                 // (level L never holds an unknown)
  const int ch = blockIdx.z;
  const Lev f = level_of(rc, l), c = level_of(rc, l + 1);
  const int tw = (f.w + kT - 1) / kT;
  const long long nt = tiles_of(f.h, f.w);
  const uint8_t* img = images + rc.ioff;
  const uint8_t* mk = masks + rc.moff;
  const float* uin = l == 0 ? (MODE == PRE ? ws.u0a : ws.u0b) : ws.ea;                    // (PUSH reads none; PRE at l >= 1 starts from zero)
  float* uout = l == 0 ? (MODE == PRE ? ws.u0b : ws.u0a) : (MODE == POST ? ws.eb : ws.ea);
  const long long cap = l == 0 ? ws.p0 : ws.pc;
  const float* csrc = MODE == PUSH ? ws.ea : ws.eb;
  for (long long tile = blockIdx.x; tile < nt; tile += gridDim.x) {
    if (!ws.tf[f.toff + tile]) continue;
    const int ty = (int)(tile / tw), tx = (int)(tile % tw);
    const int gy0 = ty * kT - kR, gx0 = tx * kT - kR;
    __syncthreads();
    for (int k = threadIdx.x; k < kS * kS; k += kThreads) {
      const int gy = gy0 + k / kS, gx = gx0 + k % kS;
      float v = 0.f, b = 0.f;
      uint8_t fl = 2;                                      // 2: outside the level
      if (gy >= 0 && gx >= 0 && gy < f.h && gx < f.w) {
        const long long p = (long long)gy * f.w + gx;
        const bool unknown = l == 0 ? mk[p] != 0 : ws.fc[f.off + p] != 0;
        fl = unknown;
        if (unknown) {
          if (MODE == PRE) v = l == 0 ? uin[ch * cap + f.off + p] : 0.f;
          if (MODE != PRE) {
            const int py = gy >> 1, px = gx >> 1, qy = other(py, gy, c.h), qx = other(px, gx, c.w);
            const float e = up4(coarse_at<MODE>(ws, csrc, c, ch, py, px), coarse_at<MODE>(ws, csrc, c, ch, py, qx),
                                coarse_at<MODE>(ws, csrc, c, ch, qy, px), coarse_at<MODE>(ws, csrc, c, ch, qy, qx));
            v = MODE == PUSH ? e : uin[ch * cap + f.off + p] + e;
          }
          if (MODE != PUSH && l > 0) b = ws.bc[ch * ws.pc + f.off + p];
        } else {
          v = l == 0 ? (float)img[p * C + ch] : MODE == PUSH ? ws.bc[ch * ws.pc + f.off + p] : 0.f;
        }
      }
      s_v[k] = v; s_b[k] = b; s_f[k] = fl;
    }
    __syncthreads();
    for (int hs = 0; hs < (MODE == PUSH ? 2 : 4); ++hs) {
      half_sweep(s_v, s_b, s_f, kS, 1, kS - 1, kS - 1, gy0, gx0, f.h, f.w, hs & 1);
      __syncthreads();
    }
    for (int k = threadIdx.x; k < kT * kT; k += kThreads) {
      const int ry = kR + k / kT, rx = kR + k % kT, i = ry * kS + rx;
      const int gy = gy0 + ry, gx = gx0 + rx;
      float r = 0.f;
      if (s_f[i] == 1) {
        uout[ch * cap + f.off + (long long)gy * f.w + gx] = s_v[i];
        if (MODE == PRE) r = residual_at(s_v, s_b, kS, i, gy, gx, f.h, f.w);
      }
      if (MODE == PRE) s_r[k] = r;
    }
    if (MODE == PRE) {
      __syncthreads();
      const int j = threadIdx.x / (kT / 2), i = threadIdx.x % (kT / 2);           // 16 x 16 coarse cells: one a thread
      const int Y = ty * (kT / 2) + j, X = tx * (kT / 2) + i;
      if (Y < c.h && X < c.w) {
        const long long P = c.off + (long long)Y * c.w + X;
        if (ws.fc[P]) {
          float s = s_r[(2 * j) * kT + 2 * i];
          const bool right = 2 * X + 1 < f.w, down = 2 * Y + 1 < f.h;
          if (right) s = s + s_r[(2 * j) * kT + 2 * i + 1];
          if (down) s = s + s_r[(2 * j + 1) * kT + 2 * i];
          if (down && right) s = s + s_r[(2 * j + 1) * kT + 2 * i + 1];
          ws.bc[ch * ws.pc + P] = s;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- the levels from s on: one workgroup per (image, channel), in LDS
// MODE PUSH: the push of levels L .. s, level s -> buffer A.  Otherwise one V(s): from buffer A of level 0 in place when s == 0,
// else from zero with the right-hand side the level below restricted, -> buffer B.  Only the levels up to the highest one with an
// unknown (`top`) do anything; the push reads v of level top + 1
template <int MODE>
__global__ void __launch_bounds__(kThreads) ip_coarse(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks, Ws ws, int s, int C) {
  __shared__ float s_v[kLdsCells], s_b[kLdsCells];
  __shared__ uint8_t s_f[kLdsCells];
  const Rec rc = ws.recs[blockIdx.x];
  if (rc.status != 0 || s >= rc.L) return;
  const unsigned lm = ws.lmask[blockIdx.x];
  if (!((lm >> s) & 1)) return;                            // no unknown at level s: none above either
  const int ch = blockIdx.y;
  int top = s;
  while (top + 1 < rc.L && ((lm >> (top + 1)) & 1)) ++top;
  const int last = MODE == PUSH ? top + 1 : top;           // levels s .. last are loaded
  const uint8_t* img = images + rc.ioff;
  const uint8_t* mk = masks + rc.moff;
  int lo[17];                                              // offsets of the levels in the LDS planes (level k at lo[k - s])
  Lev lv[17];
  {
    int acc = 0;
    for (int k = s; k <= last; ++k) { lv[k - s] = level_of(rc, k); lo[k - s] = acc; acc += lv[k - s].h * lv[k - s].w; }
    if (acc > kLdsCells) return;                           // (cannot happen: level s fits kLds x kLds)
  }
  for (int k = s; k <= last; ++k) {
    const Lev f = lv[k - s];
    const int o = lo[k - s];
    for (int p = threadIdx.x; p < f.h * f.w; p += kThreads) {
      const bool unknown = k == 0 ? mk[p] != 0 : ws.fc[f.off + p] != 0;
      float v = 0.f, b = 0.f;
      if (unknown) {
        if (MODE != PUSH && k == 0) v = ws.u0a[ch * ws.p0 + f.off + p];
        if (MODE != PUSH && k == s && k > 0) b = ws.bc[ch * ws.pc + f.off + p];
      } else {
        v = k == 0 ? (float)img[(long long)p * C + ch] : MODE == PUSH ? ws.bc[ch * ws.pc + f.off + p] : 0.f;
      }
      s_v[o + p] = v; s_b[o + p] = b; s_f[o + p] = unknown;
    }
  }
  __syncthreads();
  if (MODE != PUSH) {
    for (int k = s; k < top; ++k) {                        // down: two sweeps, the restricted residual
      const Lev f = lv[k - s], c = lv[k + 1 - s];
      float* v = s_v + lo[k - s];
      const float* b = s_b + lo[k - s];
      for (int hs = 0; hs < 4; ++hs) {
        half_sweep(v, b, s_f + lo[k - s], f.w, 0, f.h, f.w, 0, 0, f.h, f.w, hs & 1);
        __syncthreads();
      }
      for (int P = threadIdx.x; P < c.h * c.w; P += kThreads) {
        if (!s_f[lo[k + 1 - s] + P]) continue;
        const int Y = P / c.w, X = P % c.w;
        float sum = 0.f;
        for (int j = 0; j < 4; ++j) {
          const int y = 2 * Y + (j >> 1), x = 2 * X + (j & 1);
          if (y >= f.h || x >= f.w) continue;
          const float r = residual_at(v, b, f.w, y * f.w + x, y, x, f.h, f.w);
          sum = j == 0 ? r : sum + r;
        }
        s_b[lo[k + 1 - s] + P] = sum;
      }
      __syncthreads();
    }
  }
  for (int k = top; k >= s; --k) {                         // up: prolongation, then the sweeps
    const Lev f = lv[k - s];
    float* v = s_v + lo[k - s];
    if (MODE == PUSH || k < top) {
      const Lev c = lv[k + 1 - s];
      const float* cv = s_v + lo[k + 1 - s];
      for (int p = threadIdx.x; p < f.h * f.w; p += kThreads) {
        if (!s_f[lo[k - s] + p]) continue;
        const int y = p / f.w, x = p % f.w;
        const int py = y >> 1, px = x >> 1, qy = other(py, y, c.h), qx = other(px, x, c.w);
        const float e = up4(cv[py * c.w + px], cv[py * c.w + qx], cv[qy * c.w + px], cv[qy * c.w + qx]);
        v[p] = MODE == PUSH ? e : v[p] + e;
      }
      __syncthreads();
    }
    const int nhs = MODE == PUSH ? 2 : (k == top ? 8 : 4);   // V(top): its pre- and post-sweeps with nothing between them
    for (int hs = 0; hs < nhs; ++hs) {
      half_sweep(v, s_b + lo[k - s], s_f + lo[k - s], f.w, 0, f.h, f.w, 0, 0, f.h, f.w, hs & 1);
      __syncthreads();
    }
  }
  const Lev f = lv[0];
  float* dst = s == 0 ? ws.u0a : (MODE == PUSH ? ws.ea : ws.eb);
  const long long cap = s == 0 ? ws.p0 : ws.pc;
  for (int p = threadIdx.x; p < f.h * f.w; p += kThreads)
    if (s_f[p]) dst[ch * cap + f.off + p] = s_v[p];
}

// ---------------------------------------------------------------- store
// hole pixels: rint(min(max(u, 0), 255)), half to even; known pixels, and every pixel of an image with status 1 or 2: the input byte
__global__ void __launch_bounds__(kThreads) ip_store(const uint8_t* __restrict__ images, uint8_t* __restrict__ out, const uint8_t* __restrict__ masks,
                                                     Ws ws, int C, long long* __restrict__ stats) {
  const Rec rc = ws.recs[blockIdx.y];
  if (rc.status == 3) return;
  if (stats && blockIdx.x == 0 && threadIdx.x == 0 && rc.status == 0) stats[(size_t)blockIdx.y * 4 + 2] = __popc(ws.lmask[blockIdx.y]);
  const long long total = (long long)rc.h * rc.w * C;
  const uint8_t* img = images + rc.ioff;
  uint8_t* o = out + rc.ioff;
  const uint8_t* mk = masks + rc.moff;
  for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < total; q += (long long)gridDim.x * kThreads) {
    const long long p = q / C;
    const int ch = (int)(q - p * C);
    if (rc.status == 0 && mk[p]) {
      const float u = ws.u0a[ch * ws.p0 + rc.base0 + p];
      o[q] = (uint8_t)(int)rintf(fminf(fmaxf(u, 0.f), 255.f));
    } else if (o != img) {
      o[q] = img[q];
    }
  }
}

struct Plan { long long p0, pc, tc; size_t o_cnt, o_lm, o_u0a, o_u0b, o_ea, o_eb, o_bc, o_fc, o_tf, total; };

Plan plan_of(int N, size_t image_bytes, int C, int max_side) {
  Plan p;
  p.p0 = (long long)(image_bytes / (size_t)C);
  p.pc = p.p0 / 3 + (long long)N * (2ll * max_side + 40);
  p.tc = (p.p0 + p.pc) / (kT * kT) + (long long)N * (max_side / 8 + 40);
  size_t o = rup256((size_t)N * sizeof(Rec));
  p.o_cnt = o; o += rup256((size_t)N * sizeof(u64));
  p.o_lm = o; o += rup256((size_t)N * sizeof(unsigned));
  p.o_u0a = o; o += rup256((size_t)p.p0 * C * sizeof(float));
  p.o_u0b = o; o += rup256((size_t)p.p0 * C * sizeof(float));
  p.o_ea = o; o += rup256((size_t)p.pc * C * sizeof(float));
  p.o_eb = o; o += rup256((size_t)p.pc * C * sizeof(float));
  p.o_bc = o; o += rup256((size_t)p.pc * C * sizeof(float));
  p.o_fc = o; o += rup256((size_t)p.pc);
  p.o_tf = o; o += rup256((size_t)p.tc);
  p.total = o;
  return p;
}

int ceil_log2(int v) { int L = 0; while ((1 << L) < v) ++L; return L; }

}  // namespace

size_t inpaint_workspace_bytes(int N, size_t image_bytes, int C, int max_side) { return plan_of(N, image_bytes, C, max_side).total; }

int inpaint_launch_count(int cycles, int max_side) {
  const int L = ceil_log2(max_side);
  int lc = 0;
  while ((((max_side - 1) >> lc) + 1) > kLds) ++lc;
  return 3 + L + 1 + lc + cycles * (2 * lc + 1) + 1;
}

hipError_t launch_inpaint_ragged(const uint8_t* images, uint8_t* out, size_t image_bytes, const ImageDesc* img_descs, const uint8_t* masks,
                                 size_t mask_bytes, const ImageDesc* mask_descs, int N, int C, int cycles, long long max_pixels, long long rows,
                                 int max_side, long long* stats, void* wsp, hipStream_t st) {
  const Plan p = plan_of(N, image_bytes, C, max_side);
  uint8_t* base = (uint8_t*)wsp;
  Ws ws;
  ws.recs = (Rec*)base; ws.cnt = (u64*)(base + p.o_cnt); ws.lmask = (unsigned*)(base + p.o_lm);
  ws.u0a = (float*)(base + p.o_u0a); ws.u0b = (float*)(base + p.o_u0b);
  ws.ea = (float*)(base + p.o_ea); ws.eb = (float*)(base + p.o_eb); ws.bc = (float*)(base + p.o_bc);
  ws.fc = base + p.o_fc; ws.tf = base + p.o_tf;
  ws.p0 = p.p0; ws.pc = p.pc; ws.tc = p.tc;
  const int L = ceil_log2(max_side);
  int lc = 0;
  while ((((max_side - 1) >> lc) + 1) > kLds) ++lc;
  // tiles of level l of an image within the capacities: cells / 1024 + (h_l + w_l) / 32 + 1 at most; every kernel strides over the
  // tiles, so the figure only has to be sensible
  auto tiles = [&](int l) {
    const long long side = ((long long)(max_side - 1) >> l) + 1;
    long long cells = (max_pixels >> (2 * l)) + 2 * side + 1;
    if (cells > side * side) cells = side * side;
    long long g = cells / (kT * kT) + 2 * side / kT + 2;
    return (unsigned)(g > 65535 ? 65535 : g);
  };
  const dim3 block(kThreads);
  hipLaunchKernelGGL(ip_prep, dim3(1), block, 0, st, img_descs, mask_descs, ws, N, C, (long long)image_bytes, (long long)mask_bytes, max_pixels, rows,
                     max_side, stats);
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(ip_count, dim3(tiles(0), N), block, 0, st, masks, ws);
  hipLaunchKernelGGL(ip_status, dim3((N + kThreads - 1) / kThreads), block, 0, st, ws, N, stats);
  UWM_CHK(hipGetLastError());
  for (int l = 0; l < L; ++l) hipLaunchKernelGGL(ip_pull, dim3(tiles(l + 1), N), block, 0, st, images, masks, ws, l, C);
  UWM_CHK(hipGetLastError());
  hipLaunchKernelGGL(ip_coarse<PUSH>, dim3(N, C), block, 0, st, images, masks, ws, lc, C);
  for (int l = lc - 1; l >= 0; --l) hipLaunchKernelGGL(ip_tile<PUSH>, dim3(tiles(l), N, C), block, 0, st, images, masks, ws, l, C);
  UWM_CHK(hipGetLastError());
  for (int cyc = 0; cyc < cycles; ++cyc) {
    for (int l = 0; l < lc; ++l) hipLaunchKernelGGL(ip_tile<PRE>, dim3(tiles(l), N, C), block, 0, st, images, masks, ws, l, C);
    hipLaunchKernelGGL(ip_coarse<PRE>, dim3(N, C), block, 0, st, images, masks, ws, lc, C);
    for (int l = lc - 1; l >= 0; --l) hipLaunchKernelGGL(ip_tile<POST>, dim3(tiles(l), N, C), block, 0, st, images, masks, ws, l, C);
    UWM_CHK(hipGetLastError());
  }
  long long sx = (max_pixels * C + kThreads * 16 - 1) / (kThreads * 16);
  if (sx > 65535) sx = 65535;
  hipLaunchKernelGGL(ip_store, dim3((unsigned)sx, N), block, 0, st, images, out, masks, ws, C, stats);
  return hipGetLastError();
}

}  // namespace uwm
