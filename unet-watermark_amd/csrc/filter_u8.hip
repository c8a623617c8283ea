// The dataset filter (the reference's src/scripts/watermark_filter.py): how many pixels of every image of a ragged batch the model calls
// watermark.  For image i at its own size: m = close3(open3(resize(sigmoid(logits_i)) > T)), counts[i] = {pixels of m, h_i * w_i}, in ONE
// kernel plus a small sum.  The rule is stated in include/uwm.h and DESIGN.md 8h.  The probabilities are resized, NOT the logits
// (resize_prob, uwm_kernels.h): the two orders disagree between a confident and an unconfident tap.
//
// All per-image geometry is read from DEVICE memory; the grid is N * kFilterBlocks workgroups, each walking the tiles of its image with a
// stride, so a captured launch serves every batch of N images, whatever their sizes.  A tile is kFilterTileH x kFilterTileW = 32 x 120
// mask pixels inside a plane of 40 rows x 128 columns: the four passes of the morphology need a halo of 4, which in x is exactly one
// dword of four byte pixels.  The thresholded plane and the planes of the four passes stay in LDS as bytes of 0 / 255, four pixels to a
// dword, in TWO buffers that the passes write in turn ((40 + 38) rows x 32 dwords = 9984 bytes); a plane holds what the next pass wants
// outside the image (255 in front of an erosion, which ignores those pixels; 0 in front of a dilation), at the image border and not at
// the tile border.  Per mask pixel: 4 logits read through the cache (the plane [h][w] is small against the image; the halo recomputes a
// third of them), 0 bytes written, or 1 where the caller wants the mask; 8 bytes of partial count per workgroup.  post_process == 0 uses
// no LDS: a thread thresholds, stores and counts its own dword.
// Counts are integers summed in a fixed order (lanes by shuffle, waves in LDS, workgroups by count_sum_kernel): the same on every run.
#include "uwm_kernels.h"

namespace uwm {

namespace {

#include "image_common.inc"

constexpr int kPW = 128;                   // plane columns of a tile: image columns x0 - 4 .. x0 + 123, four to a dword
constexpr int kGroups = kPlaneGroups;      // dwords per plane row
constexpr int kTW = kFilterTileW;          // mask columns of a tile = plane columns 4 .. 123
constexpr int kTH = kFilterTileH;          // mask rows of a tile
constexpr int kHalo = 4;                   // erode, dilate, dilate, erode
static_assert(kTW == kPW - 2 * kHalo && kGroups * 4 == kPW && kTH % 8 == 0, "tile geometry");

__device__ __forceinline__ bool sides_ok(const ImageDesc& d) { return d.h >= 1 && d.w >= 1 && d.h <= (1 << 30) && d.w <= (1 << 30); }
// an image that is counted: sides in 1 .. 2^30 (every coordinate of a tile then fits an int) and, with a mask, a region inside it
__device__ __forceinline__ bool filter_desc_ok(const ImageDesc& d, bool with_mask, size_t mask_bytes) {
  return sides_ok(d) && (!with_mask || region_ok(d, 1, mask_bytes));
}

// pixels x .. x + 3 of row y of the H x W image: resize_prob > thr as bytes of 0 / 255; 0 for a column outside the image
__device__ __forceinline__ uint32_t threshold_px4(const float* __restrict__ b, int ld, int h, int w, float sy, float sx, int y, int x, int W,
                                                  float thr) {
  uint32_t m = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (x + k >= 0 && x + k < W && resize_prob(b, ld, h, w, sy, sx, y, x + k) > thr) m |= 0xFFu << (8 * k);
  return m;
}

__device__ __forceinline__ unsigned px_count(uint32_t v) { return (unsigned)__popc(v) >> 3; }      // bytes of 255 in a dword of 0 / 255

__global__ __launch_bounds__(256) void prob_mask_count_kernel(const float* __restrict__ logits, int ld, int h, int w,
                                                              const ImageDesc* __restrict__ descs, float thr, int post,
                                                              uint8_t* __restrict__ mask, size_t mask_bytes, long long* __restrict__ partial) {
  __shared__ uint32_t pa[kTH + 8][kGroups];            // thresholded (rows y0 - 4 ..), then the opening (rows y0 - 2 ..)
  __shared__ uint32_t pb[kTH + 6][kGroups];            // its erosion (rows y0 - 3 ..), then the closing's dilation (rows y0 - 1 ..)
  __shared__ unsigned long long wave_sum[4];
  const int n = blockIdx.x / kFilterBlocks, blk = blockIdx.x % kFilterBlocks;
  const ImageDesc d = descs[n];
  if (!filter_desc_ok(d, mask != nullptr, mask_bytes)) {                       // (uniform over the workgroup)
    if (mask && region_ok(d, 1, mask_bytes, 1, kAnySide)) {                                  // a side above 2^30 whose region still fits: zeros
      const size_t total = (size_t)d.h * d.w;
      for (size_t i = (size_t)blk * blockDim.x + threadIdx.x; i < total; i += (size_t)kFilterBlocks * blockDim.x) mask[d.offset + i] = 0;
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = 0;
    return;
  }
  const int H = d.h, W = d.w;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const float* b = logits + (size_t)n * h * w * ld;
  uint8_t* out = mask ? mask + d.offset : nullptr;
  const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
  const long long tiles = (long long)tiles_x * tiles_y;
  const int g = threadIdx.x & (kGroups - 1), r8 = threadIdx.x / kGroups;      // a plane dword of this thread: column group, row within a pass of 8
  const bool inner = g >= 1 && g <= kTW / 4;                                   // a group of mask columns
  unsigned long long cnt = 0;
  for (long long t = blk; t < tiles; t += kFilterBlocks) {
    const int y0 = (int)(t / tiles_x) * kTH, x0 = (int)(t % tiles_x) * kTW;
    const int x = x0 - kHalo + 4 * g;                                          // image column of this thread's dword
    if (!post) {                                                               // threshold, store, count: no plane needed
      for (int r = r8; r < kTH; r += 8) {
        const int y = y0 + r;
        if (!inner || y >= H || x >= W) continue;
        const uint32_t v = threshold_px4(b, ld, h, w, sy, sx, y, x, W, thr);
        if (out) store_px4(out, y, x, W, v);
        cnt += px_count(v);
      }
      continue;
    }
    const uint32_t in = column_mask(x, W);
    // 1. sigmoid, resize, threshold; 255 outside the image (the erosion ignores those)
    for (int r = r8; r < kTH + 8; r += 8) {
      const int y = y0 - 4 + r;
      pa[r][g] = (y >= 0 && y < H && in) ? (threshold_px4(b, ld, h, w, sy, sx, y, x, W, thr) | ~in) : 0xFFFFFFFFu;
    }
    __syncthreads();
    // 2. the opening's erosion: plane row r of pb = row r + 1 of pa; 0 outside the image (the dilation reads those as 0)
    for (int r = r8; r < kTH + 6; r += 8) {
      const int y = y0 - 3 + r;
      pb[r][g] = (y >= 0 && y < H) ? (cross<true>(pa, r + 1, g) & in) : 0u;
    }
    __syncthreads();
    // 3. the opening's dilation: row r of pa = row r + 1 of pb; 0 outside the image (a dilation follows)
    for (int r = r8; r < kTH + 4; r += 8) {
      const int y = y0 - 2 + r;
      pa[r][g] = (y >= 0 && y < H) ? (cross<false>(pb, r + 1, g) & in) : 0u;
    }
    __syncthreads();
    // 4. the closing's dilation: row r of pb = row r + 1 of pa; 255 outside the image (an erosion follows)
    for (int r = r8; r < kTH + 2; r += 8) {
      const int y = y0 - 1 + r;
      pb[r][g] = (y >= 0 && y < H) ? ((cross<false>(pa, r + 1, g) & in) | ~in) : 0xFFFFFFFFu;
    }
    __syncthreads();
    // 5. the closing's erosion, store and count: mask row r = row r + 1 of pb (pa is next written by the next tile's pass 1, pb behind
    //    the barrier that follows it)
    for (int r = r8; r < kTH; r += 8) {
      const int y = y0 + r;
      if (!inner || y >= H || x >= W) continue;
      const uint32_t v = cross<true>(pb, r + 1, g) & in;
      if (out) store_px4(out, y, x, W, v);
      cnt += px_count(v);
    }
  }
  // this workgroup's count: lanes, then waves, in a fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (long long)(wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3]);
}

// counts[n] = {sum of image n's partial counts, h_n * w_n}, or {0, 0} for a misfit: one thread per image
__global__ __launch_bounds__(256) void count_sum_kernel(const long long* __restrict__ partial, const ImageDesc* __restrict__ descs, int N,
                                                        int with_mask, size_t mask_bytes, long long* __restrict__ counts) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const ImageDesc d = descs[n];
  long long fg = 0, total = 0;
  if (filter_desc_ok(d, with_mask != 0, mask_bytes)) {
    for (int k = 0; k < kFilterBlocks; ++k) fg += partial[(size_t)n * kFilterBlocks + k];
    total = (long long)d.h * d.w;
  }
  counts[2 * (size_t)n] = fg;
  counts[2 * (size_t)n + 1] = total;
}

}  // namespace

size_t filter_workspace_bytes(int N) {
  if (N < 1 || N > 2147483647 / kFilterBlocks) return 0;
  return (size_t)N * kFilterBlocks * sizeof(long long);
}

hipError_t launch_prob_mask_count(const float* logits, int ld, int N, int h, int w, const ImageDesc* out_descs, float thr, int post_process,
                                  uint8_t* mask, size_t mask_bytes, long long* counts, void* workspace, size_t workspace_bytes,
                                  hipStream_t st) {
  const size_t need = filter_workspace_bytes(N);
  if (!logits || !out_descs || !counts || !workspace || need == 0 || workspace_bytes < need || h < 1 || w < 1 || ld < 1 ||
      (mask && mask_bytes < 1) || !(thr == thr) || thr - thr != 0.f || ((uintptr_t)logits & 3) ||
      (((uintptr_t)out_descs | (uintptr_t)counts | (uintptr_t)workspace) & 7))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(prob_mask_count_kernel, dim3((unsigned)(N * kFilterBlocks)), dim3(256), 0, st, logits, ld, h, w, out_descs, thr,
                     post_process, mask, mask_bytes, (long long*)workspace);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(count_sum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const long long*)workspace, out_descs, N,
                     mask ? 1 : 0, mask_bytes, counts);
  return hipGetLastError();
}

}  // namespace uwm
