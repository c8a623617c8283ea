// What the image kernels share: small integer and float32 arithmetic, the descriptor check, the block-wide scan of the prep kernels
// and the lock-free union-find of the component labellings.  Included inside the anonymous namespace of each image file (after
// uwm_kernels.h, inside namespace uwm), the way synth_stages.inc is.  Nothing here depends on the flags of the file that includes it:
// a float helper switches contraction off in its own body, so every operation is rounded on its own wherever it is compiled.

#define UWM_CHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

inline size_t rup256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---------------------------------------------------------------- arithmetic
// BORDER_REFLECT_101 (cv2.borderInterpolate) of ANY coordinate into [0, n): period 2(n - 1); n = 1 -> 0
__device__ __forceinline__ int reflect101(int c, int n) {
  if ((unsigned)c < (unsigned)n) return c;
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  int m = c % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}
// the same where one reflection is enough: -n < c < 2n - 1
__device__ __forceinline__ int reflect101_near(int c, int n) { return c < 0 ? -c : c >= n ? 2 * (n - 1) - c : c; }
// a / b rounded half to even, a >= 0, b > 0
__device__ __forceinline__ int div_rne(int a, int b) {
  int q = a / b;
  const int r2 = 2 * (a - q * b);
  if (r2 > b || (r2 == b && (q & 1))) ++q;
  return q;
}
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }
// Pillow's L from RGB
__device__ __forceinline__ int luma8(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }
// Image.blend(degenerate, image, f) on one channel value, in float32 with every rounding spelt out
__device__ __forceinline__ int blend8(int d, int v, float f) {
#pragma clang fp contract(off)
  const float t = __fadd_rn((float)d, __fmul_rn(f, __fsub_rn((float)v, (float)d)));
  if (f >= 0.f && f <= 1.f) return (int)t & 255;
  return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}
// Image.paste's blend of one channel value
__device__ __forceinline__ int blend255(int src, int dst, int al) { const int t = src * al + dst * (255 - al) + 128; return ((t >> 8) + t) >> 8; }
// an axis of CLAHE's blend: y -> (tile, next tile, weight of the next); every operation rounded on its own
__device__ __forceinline__ void clahe_axis(int y, float inv, int& t1, int& t2, float& a) {
#pragma clang fp contract(off)
  const float f = (float)y * inv - 0.5f, fl = floorf(f);
  a = f - fl;
  const int i = (int)fl;
  t1 = min(max(i, 0), 7);
  t2 = min(max(i + 1, 0), 7);
}

// ---------------------------------------------------------------- descriptors
constexpr int kAnySide = 2147483647;       // max_side of a caller that sets no upper bound on a side
// sides in min_side .. max_side, offset >= 0, offset + h*w*bytes_per_pixel <= buffer_bytes (h*w < 2^62: nothing overflows)
__device__ __forceinline__ bool region_ok(const ImageDesc& d, int bytes_per_pixel, size_t buffer_bytes, int min_side = 1, int max_side = 1 << 30) {
  if (d.h < min_side || d.w < min_side || d.h > max_side || d.w > max_side || d.offset < 0 || (unsigned long long)d.offset > buffer_bytes) return false;
  return (unsigned long long)d.h * (unsigned long long)d.w <= (buffer_bytes - (unsigned long long)d.offset) / (unsigned)bytes_per_pixel;
}

// inclusive scan of s[0 .. 255] (and, beside it, of s2[0 .. 255] where a prep sums two quantities) over a workgroup of 256 threads,
// thread t holding s[t].  Every thread of the workgroup must come here; the entries are written and read between barriers of its
// own, and the sums are complete when it returns
__device__ __forceinline__ void block_scan_incl(long long* s, int t, long long* s2 = nullptr) {
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    long long a = 0, b = 0;
    if (t >= d) { a = s[t - d]; if (s2) b = s2[t - d]; }
    __syncthreads();
    s[t] += a;
    if (s2) s2[t] += b;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- union-find with integer atomicMin
// A label array holds parent + BIAS: BIAS = 1 keeps 0 for "not in the set", BIAS = 0 keeps -1.  A parent is never greater than its
// child, so the root of a finished tree is the set's smallest index.
__device__ __forceinline__ int ld_label(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_label(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of p: parents never exceed their children, so the walk strictly descends
template <int BIAS>
__device__ __forceinline__ int uf_find(const int* lab, int p) {
  for (;;) {
    const int q = ld_label(lab + p) - BIAS;
    if (q == p) return p;
    p = q;
  }
}
// join the sets of a and b.  Every turn either ends or continues with max(a, b) strictly smaller.
template <int BIAS>
__device__ __forceinline__ void uf_union(int* lab, int a, int b) {
  for (;;) {
    a = uf_find<BIAS>(lab, a);
    b = uf_find<BIAS>(lab, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b + BIAS) - BIAS;   // a's parent as it was
    if (old == a) return;                                  // a was a root and now hangs below b
    a = old;                                               // a had got a parent meanwhile: that set still has to meet b's
  }
}

// The joins of pixel p = (x, y) of a W-wide image, itself in the set, with its left neighbour and the row above.  in_set(dy, dx)
// tells whether the pixel at (y + dy, x + dx) is in the set; it is only asked about pixels inside the image.  Runs inside a row are
// joined by the caller's initial labels, so p joins its left neighbour only where `joins_left` says that a run was cut there.  A
// pixel whose left neighbour is in the set with the set above it leaves the join with the row above to that neighbour (they share a
// run), so each stretch of vertical contact joins once.  CONN8: diagonal neighbours count.
template <bool CONN8, int BIAS, class InSet>
__device__ __forceinline__ void cc_join(int* lab, int p, int x, int y, int W, InSet in_set, bool joins_left) {
  const bool left = x > 0 && in_set(0, -1);
  if (left && joins_left) uf_union<BIAS>(lab, p, p - 1);
  if (y == 0) return;
  const bool up = in_set(-1, 0);
  const bool upl = x > 0 && in_set(-1, -1);
  const bool upr = CONN8 && x + 1 < W && in_set(-1, 1);    // (asked beside the other two: a read after the branch would wait on its own)
  if (up) {
    if (!(left && upl)) uf_union<BIAS>(lab, p, p - W);
  } else if (CONN8) {
    if (upl && !left) uf_union<BIAS>(lab, p, p - W - 1);   // (with `left`, the left pixel has `up` = upl and joins)
    if (upr) uf_union<BIAS>(lab, p, p - W + 1);
  }
}
