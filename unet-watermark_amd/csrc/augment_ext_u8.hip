// The stages of the reference's enhanced training recipe (get_enhanced_train_transform, src/utils/dataset.py:336-373) that follow the
// basic ones, on the uint8 image that augment_u8.hip leaves: tone (CLAHE on 8 x 8 tiles, or a gamma table) -> noise (GaussNoise) ->
// 3 x 3 blur (motion or Gaussian, reflect-101) -> Normalize.  The rule is stated in include/uwm.h and DESIGN.md 8e; after the host's
// parameter and table setup everything is integer work or float32 with every operation rounded on its own, so every result equals
// tests/augment_ext_ref.py bit for bit.
//
// Three passes: (1) augment_u8_kernel as it is, into a uint8 stage buffer of the workspace and into out_nchw; (2) one workgroup per
// (image, tile) of the images that draw CLAHE builds the tile's table; (3) per output pixel tone -> noise -> blur -> Normalize,
// recomputing the up-to-9 pre-blur values from the stage buffer (the noise is a pure function of seed, pixel and channel).  Every
// launch is sized from N, H, W alone and the descriptors are device memory: a captured graph serves every batch of a shape.
// Workgroups whose image does not draw a stage leave before any barrier.  The kernels only clamp: whatever a descriptor holds, no
// access leaves the stage buffer, the tables or the workspace.
#include "uwm_kernels.h"

#include <cmath>
#include <mutex>

namespace uwm {

constexpr int kExtRows = 4;                  // output rows of one workgroup, as augment_u8.hip
constexpr int kLabN = 16385;                 // entries of the tables indexed by a 14-bit fixed-point value, 0 .. 1.0 (FINV: 0 .. 2.0)
constexpr int kSigmaMax = 16383;             // noise_sigma (sigma * 256) is clamped to this: z * sigma stays inside int32

struct AugExtTables {
  int lin[256];                              // sRGB byte -> linear, 14 fraction bits
  unsigned short f[kLabN];                   // t (14 bits) -> f(t), 15 fraction bits
  int finv[kLabN];                           // f (13 bits, up to 2.0) -> t, 14 fraction bits
  unsigned char gam[kLabN];                  // linear (14 bits) -> sRGB byte
  int qn[1025];                              // standard-normal quantiles at i / 1024, 12 fraction bits; ends at Phi^-1(1 / 4096)
};

__device__ int d_lin[256];
__device__ unsigned short d_f[kLabN];
__device__ int d_finv[kLabN];
__device__ unsigned char d_gam[kLabN];
__device__ int d_qn[1025];

// ---- the tables: ONE definition, built on the host at first use (uwm_aug_lab_tables hands them out; tests/augment_ext_ref.py builds
// its own from the same formulae with exact integer comparisons).  The cube root is confirmed with integer comparisons; the two pow()
// tables and the quantiles are at least 3e-5 away from a rounding boundary in every entry (tests/test_augment_ext.py), far more
// than any libm is off.
static long long round_ratio(long long num, long long den) { return (2 * num + den) / (2 * den); }      // num >= 0, den > 0

static double normal_quantile_lower(double p) {      // x <= 0 with Phi(x) = p, by bisection on erfc
  double lo = -9.0, hi = 0.0;
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (0.5 * std::erfc(-mid * 0.70710678118654752440) < p) lo = mid; else hi = mid;
  }
  return 0.5 * (lo + hi);
}

static AugExtTables* build_tables() {
  AugExtTables* t = new AugExtTables;
  for (int v = 0; v < 256; ++v)
    t->lin[v] = v <= 10 ? (int)round_ratio(16384ll * v * 100, 255 * 1292)
                        : (int)std::llround(16384.0 * std::pow((v / 255.0 + 0.055) / 1.055, 2.4));
  for (long long i = 0; i < kLabN; ++i) {
    if (i * 1000000 <= 8856ll * 16384) { t->f[i] = (unsigned short)round_ratio(7787ll * 2 * i * 29 + 131072000ll, 29000); continue; }
    long long q = std::llround(32768.0 * std::cbrt(i / 16384.0));
    const long long rhs = i << 34;                     // q = round(32768 cbrt(i / 16384))  <=>  (2q - 1)^3 <= i 2^34 < (2q + 1)^3
    while ((2 * q - 1) * (2 * q - 1) * (2 * q - 1) > rhs) --q;
    while ((2 * q + 1) * (2 * q + 1) * (2 * q + 1) <= rhs) ++q;
    t->f[i] = (unsigned short)q;
  }
  for (long long j = 0; j < kLabN; ++j) {
    if (j * 1000000 > 206893ll * 8192) { t->finv[j] = (int)((j * j * j + (1ll << 24)) >> 25); continue; }
    const long long num = (29 * j - 32768) * 2000;
    t->finv[j] = num <= 0 ? 0 : (int)round_ratio(num, 29 * 7787);
  }
  for (long long i = 0; i < kLabN; ++i) {
    long long q = i * 10000000 <= 31308ll * 16384 ? round_ratio(255ll * 1292 * i, 1638400)
                                                   : std::llround(269.025 * std::pow(i / 16384.0, 1.0 / 2.4) - 14.025);
    t->gam[i] = (unsigned char)(q < 0 ? 0 : q > 255 ? 255 : q);
  }
  for (int i = 0; i < 512; ++i) {
    const long long q = std::llround(4096.0 * normal_quantile_lower(i ? i / 1024.0 : 1.0 / 4096.0));
    t->qn[i] = (int)q;
    t->qn[1024 - i] = (int)-q;
  }
  t->qn[512] = 0;
  return t;
}
const AugExtTables& aug_ext_tables() {
  static const AugExtTables* t = build_tables();
  return *t;
}
bool aug_ext_host_table(int which, const void** data, int* count, int* elem_bytes) {
  const AugExtTables& t = aug_ext_tables();
  switch (which) {
    case 0: *data = t.lin; *count = 256; *elem_bytes = 4; return true;
    case 1: *data = t.f; *count = kLabN; *elem_bytes = 2; return true;
    case 2: *data = t.finv; *count = kLabN; *elem_bytes = 4; return true;
    case 3: *data = t.gam; *count = kLabN; *elem_bytes = 1; return true;
    case 4: *data = t.qn; *count = 1025; *elem_bytes = 4; return true;
    default: return false;
  }
}

// ---- float32 products, sums and differences that are rounded on their own.  Without OCML's rounded operations the toolkit's
// __fmul_rn / __fadd_rn / __fsub_rn are plain operators that carry the compiler's default permission to contract, and a * b + c
// then becomes ONE fused instruction (it did: CLAHE's blend was a last bit off on tiles whose reciprocal is no power of two).
// Contraction is switched off for the rest of this file; pre_norm's fmaf is an explicit call and stays fused.
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

// ---- device helpers
namespace {
#include "image_common.inc"
}  // namespace

// lightness, the project's own integer rule: sRGB -> linear -> XYZ over the white point (rows sum to 4096) -> f()
__device__ __forceinline__ void lab_f(int r, int g, int b, int& fx, int& fy, int& fz) {
  const int lr = d_lin[r], lg = d_lin[g], lb = d_lin[b];
  fx = d_f[(1777 * lr + 1541 * lg + 778 * lb + 2048) >> 12];
  fy = d_f[(871 * lr + 2929 * lg + 296 * lb + 2048) >> 12];
  fz = d_f[(73 * lr + 448 * lg + 3575 * lb + 2048) >> 12];
}
__device__ __forceinline__ int lab_l8(int fy) {      // round((116 f - 16) * 255 / 100), f in 15 fraction bits (>= 16 / 116)
  return clamp255((2 * ((116 * fy - 524288) * 255) + 3276800) / 6553600);
}
__device__ __forceinline__ void lab_back(int fx, int fy, int fz, int l8, int& r, int& g, int& b) {
  const int fy2 = (65536 * (100 * l8 + 4080) + 29580) / 59160;
  const int ix = (min(max(fy2 + (fx - fy), 0), 65535) + 2) >> 2, iy = (fy2 + 2) >> 2, iz = (min(max(fy2 - (fy - fz), 0), 65535) + 2) >> 2;
  const long long X = d_finv[ix], Y = d_finv[iy], Z = d_finv[iz];
  const long long lr = (12615 * X - 6296 * Y - 2223 * Z + 2048) >> 12, lg = (-3773 * X + 7684 * Y + 185 * Z + 2048) >> 12,
                  lb = (217 * X - 836 * Y + 4715 * Z + 2048) >> 12;
  r = d_gam[(int)min(max(lr, 0ll), 16384ll)];
  g = d_gam[(int)min(max(lg, 0ll), 16384ll)];
  b = d_gam[(int)min(max(lb, 0ll), 16384ll)];
}

// the splitmix64 finaliser of seed + (counter + 1) * golden: a pure function of (seed, pixel, channel)
__device__ __forceinline__ unsigned long long hash64(unsigned long long seed, unsigned long long counter) {
  unsigned long long z = seed + (counter + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct ExtGeom { int th, tw; float inv_th, inv_tw, lut_scale; };      // CLAHE tile size, 1.0f / each, 255.0f / area: host float32 divisions

// The pre-blur value of pixel (y, x): stage byte -> tone -> noise.  tone: 0 none, 1 CLAHE (C = 1 or 3 only), 2 table.
template <int C>
__device__ __forceinline__ void ext_value(const uint8_t* __restrict__ simg, int W, int y, int x, int tone, const uint8_t* __restrict__ lut2,
                                          const uint8_t* __restrict__ luts, const ExtGeom& gm, int sigma, unsigned long long seed, int* v) {
  const size_t pix = (size_t)y * W + x;
  const uint8_t* p = simg + pix * C;
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = p[c];
  if (tone == 2) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = lut2[v[c]];
  } else if (tone == 1 && (C == 1 || C == 3)) {
    int fx = 0, fy = 0, fz = 0, l = v[0];
    if (C == 3) { lab_f(v[0], v[C > 1 ? 1 : 0], v[C > 2 ? 2 : 0], fx, fy, fz); l = lab_l8(fy); }
    int ty1, ty2, tx1, tx2;
    float ya, xa;
    clahe_axis(y, gm.inv_th, ty1, ty2, ya);
    clahe_axis(x, gm.inv_tw, tx1, tx2, xa);
    const float ya1 = sub_rn(1.0f, ya), xa1 = sub_rn(1.0f, xa);
    const float l11 = luts[(ty1 * 8 + tx1) * 256 + l], l12 = luts[(ty1 * 8 + tx2) * 256 + l];
    const float l21 = luts[(ty2 * 8 + tx1) * 256 + l], l22 = luts[(ty2 * 8 + tx2) * 256 + l];
    const float top = add_rn(mul_rn(l11, xa1), mul_rn(l12, xa)), bot = add_rn(mul_rn(l21, xa1), mul_rn(l22, xa));
    const int res = clamp255(__float2int_rn(add_rn(mul_rn(top, ya1), mul_rn(bot, ya))));
    if (C == 3) lab_back(fx, fy, fz, res, v[0], v[C > 1 ? 1 : 0], v[C > 2 ? 2 : 0]);
    else v[0] = res;
  }
  if (sigma > 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int r = (int)(hash64(seed, (unsigned long long)pix * 4ull + (unsigned)c) >> 40);
      const int k = r >> 14, fr = r & 16383;
      const int z = (d_qn[k] * (16384 - fr) + d_qn[k + 1] * fr) >> 12;      // standard normal, 14 fraction bits, |z| < 3.5
      v[c] = clamp255(v[c] + ((z * sigma) >> 22));                             // floor(v + g)
    }
  }
}

// what the kernels make of a descriptor: anything else than the listed values is "none"
__device__ __forceinline__ int ext_tone(const AugExtDesc* e, int H, int W, int C) {
  const int t = e->tone;
  return t == 2 ? 2 : (t == 1 && (C == 1 || C == 3) && H >= 8 && W >= 8) ? 1 : 0;
}

// Pass 2.  One workgroup = one tile of one image that draws CLAHE: 256-bin histogram of the (reflect-101 padded) tile in LDS with
// LDS integer atomics, clip, redistribute, prefix sum, 256-byte table -> luts [N][64][256].
template <int C>
__global__ __launch_bounds__(256) void augment_ext_hist_kernel(const uint8_t* __restrict__ stage, const AugExtDesc* __restrict__ ext, int H, int W,
                                                               ExtGeom gm, uint8_t* __restrict__ luts) {
  const int n = blockIdx.x >> 6, tile = blockIdx.x & 63, t = threadIdx.x;
  const AugExtDesc* __restrict__ e = ext + n;
  if (ext_tone(e, H, W, C) != 1) return;                                 // uniform, before any barrier
  __shared__ int hist[256];
  __shared__ int scan[2][256];
  __shared__ int s_excess;
  hist[t] = 0;
  if (t == 0) s_excess = 0;
  __syncthreads();
  const uint8_t* __restrict__ simg = stage + (size_t)n * H * W * C;
  const int y0 = (tile >> 3) * gm.th, x0 = (tile & 7) * gm.tw, area = gm.th * gm.tw;
  for (int i = t; i < area; i += 256) {
    const int dy = i / gm.tw, dx = i - dy * gm.tw;
    const uint8_t* p = simg + ((size_t)reflect101(y0 + dy, H) * W + reflect101(x0 + dx, W)) * C;
    int l = p[0];
    if (C == 3) { int fx, fy, fz; lab_f(p[0], p[C > 1 ? 1 : 0], p[C > 2 ? 2 : 0], fx, fy, fz); l = lab_l8(fy); }
    atomicAdd(&hist[l], 1);
  }
  __syncthreads();
  const int clip = max(e->clahe_clip, 1);
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
  luts[((size_t)n * 64 + tile) * 256 + t] = (uint8_t)clamp255(__float2int_rn(mul_rn((float)scan[cur][t], gm.lut_scale)));
}

// Pass 3.  The workgroup shape of augment_u8_kernel: kExtRows output rows of one image, lane t forms pixels t, t + 256, ... of a row.
template <int C>
__global__ __launch_bounds__(256) void augment_ext_apply_kernel(const uint8_t* __restrict__ stage, const AugExtDesc* __restrict__ ext, int H, int W,
                                                                int tiles, ExtGeom gm, PreArgs pa, const uint8_t* __restrict__ luts,
                                                                float* __restrict__ out_f, uint8_t* __restrict__ out_u8) {
  const int n = blockIdx.x / tiles, y_begin = (blockIdx.x % tiles) * kExtRows;
  const int y_end = min(y_begin + kExtRows, H);
  const AugExtDesc* __restrict__ e = ext + n;
  const int t = threadIdx.x;
  const int tone = ext_tone(e, H, W, C);
  const int sigma = min(max(e->noise_sigma, 0), kSigmaMax);
  int blur = e->blur == 1 || e->blur == 2 ? e->blur : 0;
  int wsum = 16;
  if (blur == 1) {
    wsum = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) wsum += e->blur_w[i] != 0;
    if (wsum == 0) blur = 0;
  }
  const size_t plane = (size_t)H * W;
  const uint8_t* __restrict__ simg = stage + (size_t)n * plane * C;       // 64-bit batch offset
  if ((tone | sigma | blur) == 0) {                                       // uniform, before any barrier: the stage pass's result stands
    if (out_u8) {
      uint8_t* o = out_u8 + (size_t)n * plane * C;
      const size_t b0 = (size_t)y_begin * W * C, b1 = (size_t)y_end * W * C;
      for (size_t i = b0 + t; i < b1; i += 256) o[i] = simg[i];
    }
    return;
  }
  __shared__ uint32_t lut_dw[64];
  __shared__ int s_w[9];
  if (t < 64) lut_dw[t] = ((const uint32_t*)e->lut2)[t];
  if (t < 9) s_w[t] = blur == 2 ? ((t & 1) ? 2 : t == 4 ? 4 : 1) : (e->blur_w[t] != 0);
  __syncthreads();
  const uint8_t* lut2 = (const uint8_t*)lut_dw;
  const uint8_t* __restrict__ luts_n = luts + (size_t)n * 64 * 256;
  const unsigned long long seed = e->seed;
  for (int y = y_begin; y < y_end; ++y) {
    for (int x = t; x < W; x += 256) {
      int v[C];
      if (blur == 0) {
        ext_value<C>(simg, W, y, x, tone, lut2, luts_n, gm, sigma, seed, v);
      } else {
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0;
        for (int i = 0; i < 3; ++i) {
          const int yy = reflect101(y + i - 1, H);
          for (int j = 0; j < 3; ++j) {
            const int w = s_w[3 * i + j];
            if (w == 0) continue;                                          // uniform
            ext_value<C>(simg, W, yy, reflect101(x + j - 1, W), tone, lut2, luts_n, gm, sigma, seed, v);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += w * v[c];
          }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = blur == 2 ? (acc[c] + 8) >> 4 : div_rne(acc[c], wsum);
      }
      const size_t pix = (size_t)y * W + x;
#pragma unroll
      for (int c = 0; c < C; ++c) out_f[((size_t)n * C + c) * plane + pix] = pre_norm((uint32_t)v[c], pa.mul[c], pa.add[c]);
      if (out_u8) {
        uint8_t* o = out_u8 + ((size_t)n * plane + pix) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = (uint8_t)v[c];
      }
    }
  }
}

// ---- host side
static size_t ext_stage_bytes(int N, int H, int W, int C) { return ((size_t)N * H * W * C + 255) / 256 * 256; }
size_t aug_ext_workspace_bytes(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 1 || C > 4) return 0;
  return ext_stage_bytes(N, H, W, C) + (size_t)N * 64 * 256;
}

// the tables go to each device once, at the first call there: a synchronous copy, so that call cannot be part of a stream capture
static hipError_t upload_tables(hipStream_t st) {
  static std::mutex mu;
  static unsigned long long done = 0;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev > 63) return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(mu);
  if (done >> dev & 1ull) return hipSuccess;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return hipErrorStreamCaptureUnsupported;
  const AugExtTables& t = aug_ext_tables();
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(d_lin), t.lin, sizeof(t.lin))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(d_f), t.f, sizeof(t.f))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(d_finv), t.finv, sizeof(t.finv))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(d_gam), t.gam, sizeof(t.gam))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(d_qn), t.qn, sizeof(t.qn))) != hipSuccess) return e;
  done |= 1ull << dev;
  return hipSuccess;
}

template <int C>
static void launch_ext_passes(const uint8_t* stage, const AugExtDesc* ext, int N, int H, int W, int tiles, const ExtGeom& gm, const PreArgs& pa,
                              uint8_t* luts, float* out_f, uint8_t* out_u8, hipStream_t st) {
  if ((C == 1 || C == 3) && H >= 8 && W >= 8)
    hipLaunchKernelGGL(augment_ext_hist_kernel<C>, dim3((unsigned)(N * 64)), dim3(256), 0, st, stage, ext, H, W, gm, luts);
  hipLaunchKernelGGL(augment_ext_apply_kernel<C>, dim3((unsigned)(tiles * N)), dim3(256), 0, st, stage, ext, H, W, tiles, gm, pa,
                     (const uint8_t*)luts, out_f, out_u8);
}

hipError_t launch_augment_ext(const uint8_t* img, const uint8_t* masks, const AugDesc* descs, const AugExtDesc* ext, int N, int H, int W, int C,
                              const float* mean, const float* std, int thr, void* workspace, size_t workspace_bytes, float* out_f,
                              uint8_t* out_masks, uint8_t* out_u8, hipStream_t st) {
  hipError_t e;
  if (!ext) {                                                               // uwm_augment_u8, launch for launch
    if ((e = launch_augment_u8(img, descs, N, H, W, C, mean, std, out_f, out_u8, st)) != hipSuccess) return e;
    return masks ? launch_augment_mask(masks, descs, N, H, W, thr, out_masks, st) : hipSuccess;
  }
  const size_t need = aug_ext_workspace_bytes(N, H, W, C);
  const long long tiles = ((long long)H + kExtRows - 1) / kExtRows;
  if (!need || !workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) || ((uintptr_t)ext & 7) || !mean || !std ||
      tiles * N > 2147483647ll || (long long)N * 64 > 2147483647ll)
    return hipErrorInvalidValue;
  if ((e = upload_tables(st)) != hipSuccess) return e;
  uint8_t* stage = (uint8_t*)workspace;
  uint8_t* luts = stage + ext_stage_bytes(N, H, W, C);
  if ((e = launch_augment_u8(img, descs, N, H, W, C, mean, std, out_f, stage, st)) != hipSuccess) return e;
  if (masks && (e = launch_augment_mask(masks, descs, N, H, W, thr, out_masks, st)) != hipSuccess) return e;
  ExtGeom gm;
  gm.th = (H + 7) / 8; gm.tw = (W + 7) / 8;
  gm.inv_th = 1.0f / (float)gm.th; gm.inv_tw = 1.0f / (float)gm.tw;
  gm.lut_scale = 255.0f / (float)(gm.th * gm.tw);
  const PreArgs pa = make_pre_args(C, mean, std);
  switch (C) {
    case 1: launch_ext_passes<1>(stage, ext, N, H, W, (int)tiles, gm, pa, luts, out_f, out_u8, st); break;
    case 2: launch_ext_passes<2>(stage, ext, N, H, W, (int)tiles, gm, pa, luts, out_f, out_u8, st); break;
    case 3: launch_ext_passes<3>(stage, ext, N, H, W, (int)tiles, gm, pa, luts, out_f, out_u8, st); break;
    default: launch_ext_passes<4>(stage, ext, N, H, W, (int)tiles, gm, pa, luts, out_f, out_u8, st); break;
  }
  return hipGetLastError();
}

}  // namespace uwm
