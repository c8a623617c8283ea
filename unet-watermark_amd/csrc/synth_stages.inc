// The stage arithmetic that the logo chain (synth_u8.hip) and the text chain (synth_text_u8.hip) share: Pillow's LANCZOS tables and
// resample pass, affine_fixed rotation, extended box blur, Image.blend and the paste blend, each restated operation by operation
// (include/uwm.h states the rules).  Included, after image_common.inc, inside the anonymous namespace of a file built with -ffp-contract=off.  A stage body
// works on one job's patch from workgroup `blk` of kB: thread t of that workgroup takes pixels blk*256 + t, + kB*256, ...

constexpr int kB = kSynthBlocks;
constexpr int kMaxSide = 32767;            // Pillow's affine_fixed holds below 32768; every product of two sides fits an int
constexpr int kMaxBlurR = 32;

__device__ __forceinline__ int lanczos_ksize(int in, int out) {
  const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(3.0 * fs) * 2 + 1;
}

__device__ __forceinline__ bool finite_small(double v) { return fabs(v) < 65536.0; }      // false for NaN

// ---------------------------------------------------------------------------------------------- LANCZOS tables (Pillow's precompute_coeffs)
__device__ __forceinline__ double sinc(double x) {
  if (x == 0.0) return 1.0;
  x = __dmul_rn(x, 3.14159265358979323846);
  return sin(x) / x;
}
__device__ __forceinline__ double lanczos(double x) {
  if (-3.0 <= x && x < 3.0) return __dmul_rn(sinc(x), sinc(x / 3.0));
  return 0.0;
}
// row xx of the table in -> out: {xmin, xmax, ksize coefficients of 22 bits}; two passes over the taps, the sum in Pillow's order
__device__ void lanczos_row(int in, int out, int ksize, int xx, int* __restrict__ row) {
  const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale;
  const double support = __dmul_rn(3.0, fs), ss = 1.0 / fs;
  const double center = __dmul_rn(__dadd_rn((double)xx, 0.5), scale);
  int xmin = (int)__dadd_rn(__dadd_rn(center, -support), 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)__dadd_rn(__dadd_rn(center, support), 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  if (xmax > ksize) xmax = ksize;                      // (never by the arithmetic above; keeps the row inside its table whatever happens)
  if (xmax < 0) xmax = 0;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww = __dadd_rn(ww, lanczos(__dmul_rn(__dadd_rn(__dadd_rn((double)(x + xmin), -center), 0.5), ss)));
  row[0] = xmin; row[1] = xmax;
  for (int x = 0; x < ksize; ++x) {
    int k = 0;
    if (x < xmax) {
      double w = lanczos(__dmul_rn(__dadd_rn(__dadd_rn((double)(x + xmin), -center), 0.5), ss));
      if (ww != 0.0) w = w / ww;
      const double v = __dmul_rn(w, 4194304.0);
      k = w < 0 ? (int)__dadd_rn(v, -0.5) : (int)__dadd_rn(v, 0.5);
    }
    row[2 + x] = k;
  }
}
// this workgroup's rows of the table in -> out
__device__ __forceinline__ void lanczos_rows(int in, int out, int ksize, int* __restrict__ table, int blk) {
  for (int xx = blk * 256 + threadIdx.x; xx < out; xx += kB * 256) lanczos_row(in, out, ksize, xx, table + (size_t)xx * (ksize + 2));
}

// ---------------------------------------------------------------------------------------------- one resample pass of Image.resize(LANCZOS) on RGBA
__device__ __forceinline__ int muldiv255(int x, int y) { const int t = x * y + 128; return ((t >> 8) + t) >> 8; }
__device__ __forceinline__ uint32_t pack4(int r, int g, int b, int a) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | ((uint32_t)a << 24); }

// src (sw wide) -> dst (dw x dh) along x (horiz) or y; premul: the first pass of its resize that runs, unpremul: the last one
__device__ __forceinline__ void resample_pass(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int sw, int dw, int dh,
                                              const int* __restrict__ tab, int ks, bool horiz, bool premul, bool unpremul, int blk) {
  const int total = dw * dh;
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const int y = i / dw, x = i - y * dw;
    const int* __restrict__ row = tab + (size_t)(horiz ? x : y) * (ks + 2);
    const int xmin = row[0], xmax = row[1];
    int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
    for (int k = 0; k < xmax; ++k) {
      const uint32_t v = horiz ? src[(size_t)y * sw + xmin + k] : src[(size_t)(xmin + k) * sw + x];
      int c0 = v & 255, c1 = (v >> 8) & 255, c2 = (v >> 16) & 255;
      const int c3 = v >> 24;
      if (premul) { c0 = muldiv255(c0, c3); c1 = muldiv255(c1, c3); c2 = muldiv255(c2, c3); }
      const int kk = row[2 + k];
      acc[0] += c0 * kk; acc[1] += c1 * kk; acc[2] += c2 * kk; acc[3] += c3 * kk;
    }
    int r = clamp255(acc[0] >> 22), g = clamp255(acc[1] >> 22), b = clamp255(acc[2] >> 22);
    const int al = clamp255(acc[3] >> 22);
    if (unpremul && al != 0 && al != 255) { r = min(255, 255 * r / al); g = min(255, 255 * g / al); b = min(255, 255 * b / al); }
    dst[i] = pack4(r, g, b, al);
  }
}

// ---------------------------------------------------------------------------------------------- Pillow's affine_fixed, NEAREST, fill 0
__device__ __forceinline__ long long fix16(double v) { return (long long)floor(__dadd_rn(__dmul_rn(v, 65536.0), 0.5)); }

__device__ __forceinline__ void rotate_pass(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int sw, int sh, int dw, int dh,
                                            const double* rot, int blk) {
  const long long a0 = fix16(rot[0]), a1 = fix16(rot[1]), a3 = fix16(rot[3]), a4 = fix16(rot[4]);
  const long long a2 = fix16(__dadd_rn(__dadd_rn(rot[2], __dmul_rn(rot[0], 0.5)), __dmul_rn(rot[1], 0.5)));
  const long long a5 = fix16(__dadd_rn(__dadd_rn(rot[5], __dmul_rn(rot[3], 0.5)), __dmul_rn(rot[4], 0.5)));
  const int total = dw * dh;
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const int y = i / dw, x = i - y * dw;
    const long long xin = (a2 + a1 * y + a0 * x) >> 16, yin = (a5 + a4 * y + a3 * x) >> 16;
    dst[i] = (xin >= 0 && xin < sw && yin >= 0 && yin < sh) ? src[(size_t)yin * sw + (size_t)xin] : 0u;
  }
}

// ---------------------------------------------------------------------------------------------- one extended box blur pass of GaussianBlur
__device__ __forceinline__ void blur_pass(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int w, int h, int R, unsigned long long ww,
                                          unsigned long long fw, bool horiz, int blk) {
  const int n = horiz ? w : h, step = horiz ? 1 : w;
  const int total = w * h;
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const int y = i / w, x = i - y * w;
    const int pos = horiz ? x : y;
    const uint32_t* __restrict__ line = src + (horiz ? (size_t)y * w : (size_t)x);
    unsigned acc[4] = {0u, 0u, 0u, 0u};
    for (int d = -R; d <= R; ++d) {
      const uint32_t v = line[(size_t)min(max(pos + d, 0), n - 1) * step];
      acc[0] += v & 255; acc[1] += (v >> 8) & 255; acc[2] += (v >> 16) & 255; acc[3] += v >> 24;
    }
    const uint32_t lo = line[(size_t)min(max(pos - R - 1, 0), n - 1) * step], hi = line[(size_t)min(max(pos + R + 1, 0), n - 1) * step];
    uint32_t out = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned far = ((lo >> (8 * c)) & 255) + ((hi >> (8 * c)) & 255);
      out |= (uint32_t)(((ww * acc[c] + fw * far + (1ull << 23)) >> 24) & 255ull) << (8 * c);
    }
    dst[i] = out;
  }
}

// ---------------------------------------------------------------------------------------------- ImageEnhance and paste
// this workgroup's partial sum of L over the brightened patch (the Contrast degenerate is the mean) -> *part; integer sums: any order,
// one result.  Every thread of the workgroup must come here (it synchronises)
__device__ __forceinline__ void luma_partial(const uint32_t* __restrict__ src, int total, float fb, int blk, long long* __restrict__ red,
                                             long long* __restrict__ part) {
  long long sum = 0;
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const uint32_t v = src[i];
    sum += luma8(blend8(0, v & 255, fb), blend8(0, (v >> 8) & 255, fb), blend8(0, (v >> 16) & 255, fb));
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) *part = red[0];
}
// (int)(mean(L) + 0.5) in float64 from the kB partial sums
__device__ __forceinline__ int luma_mean(const long long* __restrict__ part, int total) {
  long long sum = 0;
  for (int b = 0; b < kB; ++b) sum += part[b];
  return (int)__dadd_rn((double)sum / (double)total, 0.5);
}

