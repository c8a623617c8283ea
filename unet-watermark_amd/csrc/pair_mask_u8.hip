// Masks from watermarked / clean pairs on the device (the reference's WatermarkDataset._generate_mask, use_blurred_mask = False):
// mask = open3(gray(|wm - clean|) > T) at the image's own size, for a ragged batch, in ONE kernel.  The rule is stated in
// include/uwm.h and DESIGN.md 8g; it is integer work throughout, so every result is exact.
//
// All per-image geometry is read from DEVICE memory; the grid is N * kPairMaskBlocks workgroups, each walking the tiles of its image
// with a stride, so a captured launch serves every batch of N pairs, whatever their sizes.  Per tile the two images' rows go through
// LDS as aligned dwords (rows of 3*w bytes start on any byte), the thresholded plane, its erosion and its dilation stay in LDS as
// bytes of 0 / 255, four pixels to a dword, and only the mask tile is stored: 3 + 3 bytes read and 1 written per pixel, plus the halo.
#include "uwm_kernels.h"

namespace uwm {

namespace {

#include "image_common.inc"

constexpr int kPW = 128;                   // plane columns of a tile: image columns x0 - 4 .. x0 + 123, four to a dword
constexpr int kGroups = kPlaneGroups;      // dwords per plane row (column_mask, cross, store_px4: uwm_kernels.h)
constexpr int kTW = kPairMaskTileW;        // mask columns of a tile = plane columns 4 .. 123 (the halo of 2 is rounded up to a dword)
constexpr int kTH = kPairMaskTileH;        // mask rows of a tile
constexpr int kTRows = kTH + 4;            // thresholded plane: rows y0 - 2 .. y0 + kTH + 1
constexpr int kERows = kTH + 2;            // eroded plane:      rows y0 - 1 .. y0 + kTH
constexpr int kRawDwords = (kPW * 3 + 3 + 3) / 4;      // a staged row: 384 bytes behind up to 3 bytes of misalignment (97 dwords)
static_assert(kTW == kPW - 8 && kGroups == 32 && kRawDwords == 97, "tile geometry");

// one image row's bytes [g0, g0 + nbytes) -> LDS as aligned-down dwords, one per lane of ONE wave (coalesced); byte k of the range is
// then at ((uint8_t*)dst)[(g0 & 3) + k].  A dword that would reach past src_bytes is read byte by byte.
__device__ __forceinline__ void stage_span(const uint8_t* __restrict__ src, size_t src_bytes, size_t g0, int nbytes, uint32_t* dst, int lane) {
  const size_t al = g0 & ~(size_t)3;
  const int ndw = ((int)(g0 - al) + nbytes + 3) / 4;                // <= kRawDwords
  for (int d = lane; d < ndw; d += 64) {
    const size_t b = al + 4 * (size_t)d;
    uint32_t v = 0u;
    if (b + 4 <= src_bytes) v = *(const uint32_t*)(src + b);
    else
      for (int k = 0; k < 4; ++k) if (b + k < src_bytes) v |= (uint32_t)src[b + k] << (8 * k);
    dst[d] = v;
  }
}

// 12 bytes (four RGB pixels) that start at byte `at` of a staged row, as three dwords
struct Px4 { uint32_t d[3]; };
__device__ __forceinline__ Px4 load_px4(const uint32_t* row, int at) {
  const int i = at >> 2, sh = 8 * (at & 3);
  const uint32_t q0 = row[i], q1 = row[i + 1], q2 = row[i + 2], q3 = row[i + 3];
  Px4 p;
  p.d[0] = (uint32_t)((((uint64_t)q1 << 32) | q0) >> sh);
  p.d[1] = (uint32_t)((((uint64_t)q2 << 32) | q1) >> sh);
  p.d[2] = (uint32_t)((((uint64_t)q3 << 32) | q2) >> sh);
  return p;
}
__device__ __forceinline__ int px_byte(const Px4& p, int i) { return (int)((p.d[i >> 2] >> (8 * (i & 3))) & 0xFFu); }

// cv2.absdiff -> cvtColor(RGB2GRAY), OpenCV 4.x's 8-bit rule (15 coefficient bits) -> cv2.threshold(THRESH_BINARY): 0 / 255 per pixel
__device__ __forceinline__ uint32_t diff_gray_threshold(const Px4& a, const Px4& b, int thr) {
  uint32_t m = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int dr = abs(px_byte(a, 3 * k) - px_byte(b, 3 * k)), dg = abs(px_byte(a, 3 * k + 1) - px_byte(b, 3 * k + 1)),
              db = abs(px_byte(a, 3 * k + 2) - px_byte(b, 3 * k + 2));
    const int g = (dr * 9798 + dg * 19235 + db * 3735 + 16384) >> 15;
    if (g > thr) m |= 0xFFu << (8 * k);
  }
  return m;
}

__global__ __launch_bounds__(256) void pair_mask_u8_kernel(const uint8_t* __restrict__ wm, size_t wm_bytes, const ImageDesc* __restrict__ wm_descs,
                                                           const uint8_t* __restrict__ clean, size_t clean_bytes,
                                                           const ImageDesc* __restrict__ clean_descs, int thr, int open,
                                                           uint8_t* __restrict__ mask, size_t mask_bytes, const ImageDesc* __restrict__ mask_descs) {
  __shared__ uint32_t raw[2][kTRows][kRawDwords];      // the two images' rows of the tile, as loaded
  __shared__ uint32_t tp[kTRows][kGroups];             // gray(|wm - clean|) > T; 255 outside the image (the erosion ignores those)
  __shared__ uint32_t ep[kERows][kGroups];             // its erosion; 0 outside the image (the dilation reads those as 0)
  const int n = blockIdx.x / kPairMaskBlocks, blk = blockIdx.x % kPairMaskBlocks;
  const ImageDesc cd = clean_descs[n];
  if (cd.h == 0) return;                               // no clean image: the mask bytes stay (everything below is uniform over the workgroup)
  const ImageDesc wd = wm_descs[n], md = mask_descs[n];
  // (region_ok: h, w in 1 .. 2^30, so every coordinate of a tile fits an int)
  if (!region_ok(md, 1, mask_bytes)) return;        // nowhere to write
  uint8_t* out = mask + md.offset;
  const int h = md.h, w = md.w;
  if (!region_ok(wd, 3, wm_bytes) || !region_ok(cd, 3, clean_bytes) || wd.h != h || wd.w != w || cd.h != h || cd.w != w) {
    const size_t total = (size_t)h * w;
    for (size_t i = (size_t)blk * blockDim.x + threadIdx.x; i < total; i += (size_t)kPairMaskBlocks * blockDim.x) out[i] = 0;
    return;
  }
  const int tiles_x = (w + kTW - 1) / kTW, tiles_y = (h + kTH - 1) / kTH;
  const long long tiles = (long long)tiles_x * tiles_y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = threadIdx.x & (kGroups - 1), r8 = threadIdx.x / kGroups;      // a plane dword of this thread: column group, row within a pass of 8
  for (long long t = blk; t < tiles; t += kPairMaskBlocks) {
    const int y0 = (int)(t / tiles_x) * kTH, x0 = (int)(t % tiles_x) * kTW;
    const int xs = x0 - 4;                                                    // image column of plane column 0
    const int cx0 = max(xs, 0), cx1 = min(xs + kPW, w);                       // the image columns the tile reads
    // 1. the rows of both images -> LDS, one wave per row
    for (int r = wave; r < kTRows; r += 4) {
      const int y = y0 - 2 + r;
      if (y < 0 || y >= h) continue;
      const size_t px = (size_t)y * w + cx0;
      stage_span(wm, wm_bytes, (size_t)wd.offset + px * 3, (cx1 - cx0) * 3, raw[0][r], lane);
      stage_span(clean, clean_bytes, (size_t)cd.offset + px * 3, (cx1 - cx0) * 3, raw[1][r], lane);
    }
    __syncthreads();
    // 2. difference, gray, threshold
    for (int r = r8; r < kTRows; r += 8) {
      const int y = y0 - 2 + r, x = xs + 4 * g;
      uint32_t v = 0xFFFFFFFFu;
      if (y >= 0 && y < h && x >= cx0 && x < cx1) {                           // (x < 0 only as the whole first group of the first tile column)
        const size_t px = (size_t)y * w + cx0;
        const int aw = (int)(((size_t)wd.offset + px * 3) & 3), ac = (int)(((size_t)cd.offset + px * 3) & 3);
        const uint32_t in = column_mask(x, w);
        v = (diff_gray_threshold(load_px4(raw[0][r], aw + (x - cx0) * 3), load_px4(raw[1][r], ac + (x - cx0) * 3), thr) & in) | ~in;
      }
      tp[r][g] = v;
    }
    __syncthreads();
    if (!open) {                                                              // steps 2-4 of the rule only
      for (int r = r8; r < kTH; r += 8) {
        const int y = y0 + r, x = x0 + 4 * (g - 1);
        if (g >= 1 && g <= kTW / 4 && y < h) store_px4(out, y, x, w, tp[r + 2][g]);
      }
      continue;                                                               // (tp is next written behind the next tile's barrier)
    }
    // 3. erode: plane row r of ep = row r + 1 of tp
    for (int r = r8; r < kERows; r += 8) {
      const int y = y0 - 1 + r;
      ep[r][g] = (y >= 0 && y < h) ? (cross<true>(tp, r + 1, g) & column_mask(xs + 4 * g, w)) : 0u;
    }
    __syncthreads();
    // 4. dilate and store: mask row r = row r + 1 of ep
    for (int r = r8; r < kTH; r += 8) {
      const int y = y0 + r, x = x0 + 4 * (g - 1);
      if (g >= 1 && g <= kTW / 4 && y < h) store_px4(out, y, x, w, cross<false>(ep, r + 1, g));
    }
  }
}

}  // namespace

hipError_t launch_pair_mask_u8(const uint8_t* wm, size_t wm_bytes, const ImageDesc* wm_descs, const uint8_t* clean, size_t clean_bytes,
                               const ImageDesc* clean_descs, int N, int threshold, int open, uint8_t* mask, size_t mask_bytes,
                               const ImageDesc* mask_descs, hipStream_t st) {
  if (!wm || !wm_descs || !clean || !clean_descs || !mask || !mask_descs || wm_bytes < 1 || clean_bytes < 1 || mask_bytes < 1 || N < 1 ||
      (long long)N * kPairMaskBlocks > 2147483647ll || threshold < 0 || threshold > 255 || (((uintptr_t)wm | (uintptr_t)clean) & 3) ||
      (((uintptr_t)wm_descs | (uintptr_t)clean_descs | (uintptr_t)mask_descs) & 7))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pair_mask_u8_kernel, dim3((unsigned)(N * kPairMaskBlocks)), dim3(256), 0, st, wm, wm_bytes, wm_descs, clean, clean_bytes,
                     clean_descs, threshold, open, mask, mask_bytes, mask_descs);
  return hipGetLastError();
}

}  // namespace uwm
