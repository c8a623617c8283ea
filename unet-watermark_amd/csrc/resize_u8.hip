// cv2-convention resize of a ragged batch of uint8 images on the device (the reference's A.Resize(IMG_SIZE, IMG_SIZE):
// cv2.resize INTER_LINEAR on the image, INTER_NEAREST on the mask), alone, fused with Normalize into the forward's NHWC4 input, and
// the way back: one logit plane per image resized to each image's own size and thresholded.  The rule is stated in include/uwm.h
// and DESIGN.md 8c; it is integer work after the tap computation, so every result is exact.
//
// All per-image geometry (offset, h, w) is read from DEVICE memory by the kernels; every grid is sized from N, H, W (model side) or
// from a fixed block count per image (output side).  A captured launch therefore serves every batch of N images, whatever their sizes.
#include "uwm_kernels.h"

namespace uwm {

typedef float f4 __attribute__((ext_vector_type(4)));

namespace {
#include "image_common.inc"
}  // namespace

// ---------------------------------------------------------------- taps of one axis
// INTER_LINEAR, 11 coefficient bits: source index pair (s, s1) and the weights a0 + a1 (= 2048 up to the rounding of 1 - f).
// The double expression is evaluated as written — multiply, then subtract, each rounded — which a fused multiply-add would not do.
struct LinTap { int s, s1, a0, a1; };
__device__ __forceinline__ double axis_scale(int dst, int src) { return 1.0 / ((double)dst / (double)src); }      // in this order
__device__ __forceinline__ LinTap linear_tap(int d, double scale, int src) {
#pragma clang fp contract(off)
  const double p = ((double)d + 0.5) * scale;
  float f = (float)(p - 0.5);
  const float fl = floorf(f);
  int s = (int)fl;
  f -= fl;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= src - 1) { f = 0.f; s = src - 1; }
  LinTap t;
  t.s = s; t.s1 = min(s + 1, src - 1);
  t.a1 = (int)rintf(f * 2048.f);                 // round half to even
  t.a0 = (int)rintf((1.f - f) * 2048.f);
  return t;
}
// INTER_NEAREST: floor(d * scale), clamped
__device__ __forceinline__ int nearest_tap(int d, double scale, int src) {
#pragma clang fp contract(off)
  const double p = floor((double)d * scale);
  return p < (double)(src - 1) ? (int)p : src - 1;
}
// VResizeLinear's 8-bit rule on two horizontally interpolated sums
__device__ __forceinline__ int vlin(int S0, int S1, int b0, int b1) {
  return (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
}

constexpr int kRowsPerBlock = kResizeRowsPerBlock;      // output rows of one workgroup
constexpr int kRowBytes = 16384;          // widest source row (w*C bytes) staged through LDS; wider rows are gathered from global memory
constexpr int kRowDwords = kRowBytes / 4 + 1;      // (+1: a row that does not start on a dword boundary)
enum { kModeNearest = 0, kModeLinear = 1, kModeLinearNorm = 2 };

// one source row -> LDS as aligned-down dwords, one per lane (coalesced); byte k of the row is then at ((uint8_t*)dst)[(g0 & 3) + k].
// The last dword of the buffer is read byte by byte where it would reach past src_bytes.
__device__ __forceinline__ void stage_row(const uint8_t* __restrict__ src, size_t src_bytes, size_t g0, int row_bytes, uint32_t* dst) {
  const size_t al = g0 & ~(size_t)3;
  const int ndw = (int)((g0 - al) + (size_t)row_bytes + 3) / 4;
  for (int d = threadIdx.x; d < ndw; d += blockDim.x) {
    const size_t b = al + 4 * (size_t)d;
    uint32_t v = 0u;
    if (b + 4 <= src_bytes) v = *(const uint32_t*)(src + b);
    else
      for (int k = 0; k < 4; ++k) if (b + k < src_bytes) v |= (uint32_t)src[b + k] << (8 * k);
    dst[d] = v;
  }
}

// the pixels of one output row from its two source rows r0 / r1 (LDS or global memory: byte k of the row at r[k])
template <int C, int MODE, typename Row>
__device__ __forceinline__ void row_pixels(Row r0, Row r1, int b0, int b1, double scale_x, int w, int W, const PreArgs& pa,
                                           uint8_t* __restrict__ out_u8, float* __restrict__ out_f) {
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    int v[4] = {0, 0, 0, 0};
    if (MODE == kModeNearest) {
      const int ix = nearest_tap(x, scale_x, w);
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = r0[(size_t)ix * C + c];
    } else {
      const LinTap t = linear_tap(x, scale_x, w);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const size_t i0 = (size_t)t.s * C + c, i1 = (size_t)t.s1 * C + c;
        const int S0 = (int)r0[i0] * t.a0 + (int)r0[i1] * t.a1;
        const int S1 = (int)r1[i0] * t.a0 + (int)r1[i1] * t.a1;
        v[c] = vlin(S0, S1, b0, b1);
      }
    }
    if (MODE == kModeLinearNorm) {
      f4 o; o.x = 0.f; o.y = 0.f; o.z = 0.f; o.w = 0.f;
      o.x = pre_norm((uint32_t)v[0], pa.mul[0], pa.add[0]);
      if (C > 1) o.y = pre_norm((uint32_t)v[1], pa.mul[1], pa.add[1]);
      if (C > 2) o.z = pre_norm((uint32_t)v[2], pa.mul[2], pa.add[2]);
      if (C > 3) o.w = pre_norm((uint32_t)v[3], pa.mul[3], pa.add[3]);
      __builtin_nontemporal_store(o, (f4*)(out_f + (size_t)x * 4));
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) out_u8[(size_t)x * C + c] = (uint8_t)v[c];
    }
  }
}

// One workgroup = kRowsPerBlock consecutive output rows of one image.  Per output row it stages the two source rows (one for
// nearest) through LDS and every lane then forms pixels x = t, t + 256, ...; taps are recomputed per pixel (a dozen VALU operations
// beside 16 bytes stored).  A source row pair that the previous output row already staged (upscales) is kept.  An image whose
// descriptor would read outside the buffer gives zeros.
template <int C, int MODE>
__global__ __launch_bounds__(256) void resize_u8_kernel(const uint8_t* __restrict__ src, size_t src_bytes, const ImageDesc* __restrict__ descs,
                                                        int H, int W, int tiles, PreArgs pa, uint8_t* __restrict__ out_u8,
                                                        float* __restrict__ out_f) {
  __shared__ uint32_t rows[2][kRowDwords];
  const int n = blockIdx.x / tiles, y_begin = (blockIdx.x % tiles) * kRowsPerBlock;
  const int y_end = min(y_begin + kRowsPerBlock, H);
  const ImageDesc d = descs[n];
  const bool ok = region_ok(d, C, src_bytes, 1, kAnySide);       // every read of the image stays inside [0, src_bytes)
  const int h = ok ? d.h : 1, w = ok ? d.w : 1;
  const size_t base = ok ? (size_t)d.offset : 0;
  const size_t row_bytes = (size_t)w * C;
  const bool in_lds = row_bytes <= (size_t)kRowBytes;
  const double scale_y = axis_scale(H, h), scale_x = axis_scale(W, w);
  int have0 = -1, have1 = -1;
  for (int y = y_begin; y < y_end; ++y) {
    const size_t o = ((size_t)n * H + y) * W;
    uint8_t* ou = MODE == kModeLinearNorm ? nullptr : out_u8 + o * C;
    float* of = MODE == kModeLinearNorm ? out_f + o * 4 : nullptr;
    if (!ok) {                                    // (uniform over the workgroup)
      for (int x = threadIdx.x; x < W; x += blockDim.x) {
        if (MODE == kModeLinearNorm) { f4 z; z.x = z.y = z.z = z.w = 0.f; *(f4*)(of + (size_t)x * 4) = z; }
        else
          for (int c = 0; c < C; ++c) ou[(size_t)x * C + c] = 0;
      }
      continue;
    }
    int s0, s1, b0 = 2048, b1 = 0;
    if (MODE == kModeNearest) s0 = s1 = nearest_tap(y, scale_y, h);
    else { const LinTap t = linear_tap(y, scale_y, h); s0 = t.s; s1 = t.s1; b0 = t.a0; b1 = t.a1; }
    const size_t g0 = base + (size_t)s0 * row_bytes, g1 = base + (size_t)s1 * row_bytes;
    if (in_lds) {
      if (s0 != have0 || s1 != have1) {
        __syncthreads();                          // the previous row's readers are done
        stage_row(src, src_bytes, g0, (int)row_bytes, rows[0]);
        if (s1 != s0) stage_row(src, src_bytes, g1, (int)row_bytes, rows[1]);
        __syncthreads();
        have0 = s0; have1 = s1;
      }
      const uint8_t* r0 = (const uint8_t*)rows[0] + (g0 & 3);
      const uint8_t* r1 = s1 != s0 ? (const uint8_t*)rows[1] + (g1 & 3) : r0;
      row_pixels<C, MODE>(r0, r1, b0, b1, scale_x, w, W, pa, ou, of);
    } else {
      row_pixels<C, MODE>(src + g0, src + g1, b0, b1, scale_x, w, W, pa, ou, of);
    }
  }
}

template <int MODE>
static hipError_t launch_mode(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int N, int C, int H, int W, const PreArgs& pa,
                              uint8_t* out_u8, float* out_f, hipStream_t st) {
  const int tiles = (H + kRowsPerBlock - 1) / kRowsPerBlock;
  if ((long long)tiles * N > 2147483647ll) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(tiles * N)), block(256);
  switch (C) {
    case 1: hipLaunchKernelGGL((resize_u8_kernel<1, MODE>), grid, block, 0, st, src, src_bytes, descs, H, W, tiles, pa, out_u8, out_f); break;
    case 2: hipLaunchKernelGGL((resize_u8_kernel<2, MODE>), grid, block, 0, st, src, src_bytes, descs, H, W, tiles, pa, out_u8, out_f); break;
    case 3: hipLaunchKernelGGL((resize_u8_kernel<3, MODE>), grid, block, 0, st, src, src_bytes, descs, H, W, tiles, pa, out_u8, out_f); break;
    default: hipLaunchKernelGGL((resize_u8_kernel<4, MODE>), grid, block, 0, st, src, src_bytes, descs, H, W, tiles, pa, out_u8, out_f); break;
  }
  return hipGetLastError();
}
static bool bad_resize_args(const void* src, size_t src_bytes, const void* descs, int N, int C, int H, int W, const void* out) {
  return !src || !descs || !out || src_bytes < 1 || N < 1 || C < 1 || C > 4 || H < 1 || W < 1 || ((uintptr_t)src & 3) || ((uintptr_t)descs & 7);
}
hipError_t launch_resize_u8(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int N, int C, int H, int W, int interp,
                            uint8_t* out, hipStream_t st) {
  if (bad_resize_args(src, src_bytes, descs, N, C, H, W, out) || (interp != 0 && interp != 1)) return hipErrorInvalidValue;
  PreArgs pa = {};
  return interp ? launch_mode<kModeLinear>(src, src_bytes, descs, N, C, H, W, pa, out, nullptr, st)
                : launch_mode<kModeNearest>(src, src_bytes, descs, N, C, H, W, pa, out, nullptr, st);
}
hipError_t launch_resize_norm_u8_nhwc4(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int N, int C, int H, int W,
                                       const float* mean, const float* std, float* out, hipStream_t st) {
  if (bad_resize_args(src, src_bytes, descs, N, C, H, W, out) || !mean || !std || ((uintptr_t)out & 15)) return hipErrorInvalidValue;
  return launch_mode<kModeLinearNorm>(src, src_bytes, descs, N, C, H, W, make_pre_args(C, mean, std), nullptr, out, st);
}

// ---------------------------------------------------------------- the way back: logits -> each image's own size, thresholded
// kRaggedBlocks workgroups per image walk its H_i x W_i pixels with a grid stride; the pixel is resize_threshold_kernel's
// (resize_logit).  An image whose mask would not fit [0, mask_bytes) is skipped.
constexpr int kRaggedBlocks = 64;
__global__ __launch_bounds__(256) void resize_threshold_ragged_kernel(const float* __restrict__ logits, int ld, int h, int w,
                                                                      const ImageDesc* __restrict__ descs, float thr, int apply_sigmoid,
                                                                      uint8_t* __restrict__ mask, size_t mask_bytes) {
  const int n = blockIdx.x / kRaggedBlocks, blk = blockIdx.x % kRaggedBlocks;
  const ImageDesc d = descs[n];
  if (!region_ok(d, 1, mask_bytes, 1, kAnySide)) return;
  const int H = d.h, W = d.w;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const float* b = logits + (size_t)n * h * w * ld;
  uint8_t* out = mask + d.offset;
  const size_t total = (size_t)H * W;
  for (size_t i = blk * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)kRaggedBlocks * blockDim.x) {
    const int X = (int)(i % W), Y = (int)(i / W);
    const float v = resize_logit(b, ld, h, w, sy, sx, Y, X, apply_sigmoid);
    out[i] = v > thr ? 255 : 0;
  }
}
hipError_t launch_resize_threshold_ragged(const float* logits, int ld, int N, int h, int w, const ImageDesc* out_descs, float thr,
                                          int apply_sigmoid, uint8_t* mask, size_t mask_bytes, hipStream_t st) {
  if (!logits || !out_descs || !mask || mask_bytes < 1 || N < 1 || h < 1 || w < 1 || ld < 1 || ((uintptr_t)out_descs & 7) ||
      (long long)N * kRaggedBlocks > 2147483647ll)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(resize_threshold_ragged_kernel, dim3((unsigned)(N * kRaggedBlocks)), dim3(256), 0, st, logits, ld, h, w, out_descs,
                     thr, apply_sigmoid, mask, mask_bytes);
  return hipGetLastError();
}

}  // namespace uwm
