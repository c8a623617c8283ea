// Train-time augmentation of a uint8 batch on the device, one pass per tensor: flips / rot90 -> affine warp -> per-value table
// (brightness / contrast) -> HueSaturationValue -> Normalize for the image, and the same flips / rot90 -> nearest warp -> threshold
// for the mask (the reference's basic recipe, src/utils/dataset.py:375-387).  The rule is stated in include/uwm.h and DESIGN.md 8d:
// after the float64 coordinate setup everything is integer work, so every result is exact.
//
// The warp is an inverse-map gather, so the stages are composed backwards: output (x, y) -> fixed-point coordinates in the flipped
// and rotated image -> taps, each reflected into it (reflect-101) -> aug_src, the index map of uwm_preprocess_u8, into the input.
// All per-image parameters (uwm_aug_desc) are read from DEVICE memory and the grid is sized from N, H alone: a captured launch
// serves every batch of that shape.  The kernels only clamp: whatever a descriptor holds, no access leaves the image.
#include "uwm_kernels.h"

namespace uwm {

namespace {
#include "image_common.inc"
}  // namespace

constexpr int kAugRows = 4;                 // output rows of one workgroup: grid = N * ceil(H / kAugRows)
constexpr double kAugCoordMax = 1073739776.0;      // 2^30 - 2048: two clamped terms and the rounding offset still add up inside int32

// rint (round half to even) of v * 1024 as an int, clamped; a NaN gives the lower bound (fmax / fmin return the other operand)
__device__ __forceinline__ int fix10(double v) {
  return (int)fmin(fmax(rint(__dmul_rn(v, 1024.0)), -kAugCoordMax), kAugCoordMax);
}
// a * x and a * y + b with every product and sum rounded on its own (no fused multiply-add: it would change the last bit of some
// coordinates, and only for some matrices)
__device__ __forceinline__ int fix10_mul(double a, int x) { return fix10(__dmul_rn(a, (double)x)); }
__device__ __forceinline__ int fix10_mad(double a, int y, double b) { return fix10(__dadd_rn(__dmul_rn(a, (double)y), b)); }

// OpenCV's 8-bit RGB -> HSV (H in 0..179), the three shifts, and the project's integer way back (include/uwm.h)
__device__ __forceinline__ void hsv_shift(int& r, int& g, int& b, int hue, int sat, int val, const int* __restrict__ sdiv,
                                          const int* __restrict__ hdiv) {
  const int v0 = max(r, max(g, b)), d = v0 - min(r, min(g, b));
  int s = (d * sdiv[v0] + 2048) >> 12;
  const int h0 = v0 == r ? g - b : v0 == g ? b - r + 2 * d : r - g + 4 * d;
  int h = (h0 * hdiv[d] + 2048) >> 12;
  if (h < 0) h += 180;
  h = (h + hue) % 180;
  if (h < 0) h += 180;
  s = min(max(s + sat, 0), 255);
  const int v = min(max(v0 + val, 0), 255);
  const int sec = h / 30, f = h - 30 * sec;
  const int p = (v * (255 - s) + 127) / 255;
  const int q = (v * (7650 - s * f) + 3825) / 7650;
  const int t = (v * (7650 - s * (30 - f)) + 3825) / 7650;
  switch (sec) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// One workgroup = kAugRows consecutive output rows of one image; lane t forms pixels x = t, t + 256, ... of a row, so the fp32
// stores of a wave cover 256 consecutive bytes of each channel plane.  The descriptor's scalars are uniform loads (n comes from
// blockIdx), its 256-byte table goes to LDS once (64 dwords), and so do the two HSV division tables when the image shifts HSV.
// A pixel whose coordinates fall on the grid (every pixel of an image without an affine stage) takes one tap instead of four.
template <int C>
__global__ __launch_bounds__(256) void augment_u8_kernel(const uint8_t* __restrict__ img, const AugDesc* __restrict__ descs, int H, int W,
                                                         int tiles, PreArgs pa, float* __restrict__ out_f, uint8_t* __restrict__ out_u8) {
  __shared__ uint32_t lut_dw[64];
  __shared__ int sdiv[256], hdiv[256];
  const int n = blockIdx.x / tiles, y_begin = (blockIdx.x % tiles) * kAugRows;
  const int y_end = min(y_begin + kAugRows, H);
  const AugDesc* __restrict__ d = descs + n;
  const int t = threadIdx.x;
  if (t < 64) lut_dw[t] = ((const uint32_t*)d->lut)[t];
  const int flags = H == W ? d->flags : d->flags & 3;                 // (rot90 of a non-square image is refused by the callers)
  const int hue = d->hue, sat = d->sat, val = d->val;
  const bool hsv = C == 3 && (hue | sat | val) != 0;                 // uniform over the workgroup
  if (hsv) {
    sdiv[t] = t ? div_rne(255 << 12, t) : 0;
    hdiv[t] = t ? div_rne(180 << 12, 6 * t) : 0;
  }
  __syncthreads();
  const uint8_t* lut = (const uint8_t*)lut_dw;
  const double m0 = d->minv[0], m1 = d->minv[1], m2 = d->minv[2], m3 = d->minv[3], m4 = d->minv[4], m5 = d->minv[5];
  const uint8_t* __restrict__ src = img + (size_t)n * H * W * C;       // 64-bit batch offset; everything below stays inside one image
  const size_t plane = (size_t)H * W;
  for (int y = y_begin; y < y_end; ++y) {
    const int X0 = fix10_mad(m1, y, m2) + 16, Y0 = fix10_mad(m4, y, m5) + 16;
    for (int x = t; x < W; x += 256) {
      const int X = (X0 + fix10_mul(m0, x)) >> 5, Y = (Y0 + fix10_mul(m3, x)) >> 5;
      const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
      int v[C];
      int iy, ix;
      aug_src(flags, H, W, reflect101(sy, H), reflect101(sx, W), iy, ix);
      const uint8_t* p00 = src + ((size_t)iy * W + ix) * C;
      if ((fx | fy) == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = p00[c];
      } else {
        const int rx1 = reflect101(sx + 1, W), ry1 = reflect101(sy + 1, H);
        aug_src(flags, H, W, reflect101(sy, H), rx1, iy, ix);
        const uint8_t* p01 = src + ((size_t)iy * W + ix) * C;
        aug_src(flags, H, W, ry1, reflect101(sx, W), iy, ix);
        const uint8_t* p10 = src + ((size_t)iy * W + ix) * C;
        aug_src(flags, H, W, ry1, rx1, iy, ix);
        const uint8_t* p11 = src + ((size_t)iy * W + ix) * C;
        const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 512) >> 10;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = lut[v[c]];
      if (C == 3 && hsv) hsv_shift(v[0], v[C > 1 ? 1 : 0], v[C > 2 ? 2 : 0], hue, sat, val, sdiv, hdiv);
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

// the mask: nearest tap of the same map (rounding offset 512, 10 fraction bits dropped at once), then > thr
__global__ __launch_bounds__(256) void augment_mask_kernel(const uint8_t* __restrict__ m, const AugDesc* __restrict__ descs, int H, int W,
                                                           int tiles, int thr, uint8_t* __restrict__ out) {
  const int n = blockIdx.x / tiles, y_begin = (blockIdx.x % tiles) * kAugRows;
  const int y_end = min(y_begin + kAugRows, H);
  const AugDesc* __restrict__ d = descs + n;
  const int flags = H == W ? d->flags : d->flags & 3;
  const double m0 = d->minv[0], m1 = d->minv[1], m2 = d->minv[2], m3 = d->minv[3], m4 = d->minv[4], m5 = d->minv[5];
  const size_t plane = (size_t)H * W;
  const uint8_t* __restrict__ src = m + (size_t)n * plane;
  for (int y = y_begin; y < y_end; ++y) {
    const int X0 = fix10_mad(m1, y, m2) + 512, Y0 = fix10_mad(m4, y, m5) + 512;
    for (int x = threadIdx.x; x < W; x += 256) {
      const int sx = (X0 + fix10_mul(m0, x)) >> 10, sy = (Y0 + fix10_mul(m3, x)) >> 10;
      int iy, ix;
      aug_src(flags, H, W, reflect101(sy, H), reflect101(sx, W), iy, ix);
      out[(size_t)n * plane + (size_t)y * W + x] = src[(size_t)iy * W + ix] > thr ? 1 : 0;
    }
  }
}

static bool aug_grid(int N, int H, int W, int& tiles) {
  if (N < 1 || H < 1 || W < 1) return false;
  tiles = (H + kAugRows - 1) / kAugRows;
  return (long long)tiles * N <= 2147483647ll;
}
hipError_t launch_augment_u8(const uint8_t* img, const AugDesc* descs, int N, int H, int W, int C, const float* mean, const float* std,
                             float* out_f, uint8_t* out_u8, hipStream_t st) {
  int tiles;
  if (!img || !descs || !out_f || !mean || !std || C < 1 || C > 4 || ((uintptr_t)descs & 7) || !aug_grid(N, H, W, tiles)) return hipErrorInvalidValue;
  const PreArgs pa = make_pre_args(C, mean, std);
  const dim3 grid((unsigned)(tiles * N)), block(256);
  switch (C) {
    case 1: hipLaunchKernelGGL(augment_u8_kernel<1>, grid, block, 0, st, img, descs, H, W, tiles, pa, out_f, out_u8); break;
    case 2: hipLaunchKernelGGL(augment_u8_kernel<2>, grid, block, 0, st, img, descs, H, W, tiles, pa, out_f, out_u8); break;
    case 3: hipLaunchKernelGGL(augment_u8_kernel<3>, grid, block, 0, st, img, descs, H, W, tiles, pa, out_f, out_u8); break;
    default: hipLaunchKernelGGL(augment_u8_kernel<4>, grid, block, 0, st, img, descs, H, W, tiles, pa, out_f, out_u8); break;
  }
  return hipGetLastError();
}
hipError_t launch_augment_mask(const uint8_t* m, const AugDesc* descs, int N, int H, int W, int thr, uint8_t* out, hipStream_t st) {
  int tiles;
  if (!m || !descs || !out || ((uintptr_t)descs & 7) || !aug_grid(N, H, W, tiles)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(augment_mask_kernel, dim3((unsigned)(tiles * N)), dim3(256), 0, st, m, descs, H, W, tiles, thr, out);
  return hipGetLastError();
}

}  // namespace uwm
