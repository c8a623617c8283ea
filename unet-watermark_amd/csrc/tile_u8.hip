// Prediction at native resolution (include/uwm.h): a ragged batch of uint8 images is cut into model-sized overlapping
// tiles (the gather, fused with Normalize into the forward's NHWC4 input), every tile goes through the eval forward, and the tile
// logits are blended back into one plane per image at the image's own size and thresholded (the blend).  Between the two, the logit
// plane of every tile is copied out of the forward's [N][T_h][T_w][CP] output into the dense tile-logit store [K][T_h][T_w].
//
// The tile table and the per-image plans are read from DEVICE memory and checked there; every grid is sized from K, T_h, T_w or
// from a fixed block count per image.  A captured launch therefore serves every batch with the same number of tiles, whatever the
// image sizes.  The blend is a gather: one thread per output pixel sums the tiles that cover it in a fixed order, so there is no
// float atomic and a result does not depend on the schedule.
#include "uwm_kernels.h"

namespace uwm {

typedef float f4 __attribute__((ext_vector_type(4)));

namespace {
#include "image_common.inc"

// tiles along one axis of length len (>= 1), tile side T, stride S = T - overlap (>= 1): tiling.axis_count
__device__ __forceinline__ int axis_tiles(int len, int T, int S) { return len <= T ? 1 : (len - T + S - 1) / S + 1; }
// origin of tile j of n along that axis: j * S, the last one at len - T (n == 1: 0)
__device__ __forceinline__ int axis_origin(int j, int n, int len, int T, int S) { return n == 1 ? 0 : j == n - 1 ? len - T : j * S; }
// the tiles [lo, hi] of that axis that cover coordinate p (0 <= p < len), by arithmetic: tiles 0 .. n-2 start at j * S, so tile j
// covers p where j * S <= p < j * S + T; the last tile covers p >= len - T.  Consecutive tiles leave no gap (S <= T and
// len - T <= (n - 1) * S), so lo <= hi
__device__ __forceinline__ void axis_cover(int p, int n, int len, int T, int S, int& lo, int& hi) {
  if (n == 1) { lo = hi = 0; return; }
  hi = p >= len - T ? n - 1 : p / S;
  lo = p < T ? 0 : min((p - T) / S + 1, n - 1);
}
// the blend weight along one axis at coordinate t inside a tile of side T: 1 at the rim, rising by 1 per pixel towards the middle
__device__ __forceinline__ int axis_weight(int t, int T) { return min(t + 1, T - t); }
// One float32 operation, rounded on its own.  Written as plain operators under a pragma of their own: the header's __fmul_rn /
// __fadd_rn are plain operators too, but compiled where contraction is allowed, and once inlined into the blend's loop the pair
// became one v_fmac_f32 (seen in the ISA, and in the last bit of the result).  The opaque value between the two keeps the product
// a value of its own whatever the caller's flags are.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float div_rn(float a, float b) {      // IEEE division (hipcc's default: correctly rounded)
#pragma clang fp contract(off)
  return a / b;
}
}  // namespace

// ---------------------------------------------------------------- the gather: tiles of the images, normalised, as the forward's input
// One workgroup = kTileRowsPerBlock consecutive rows of one tile; lane t forms pixels x = t, t + 256, ... of a row (16 bytes stored
// per pixel, whole lines per wave).  The source coordinate is the tile origin plus (y, x), brought back into the image by
// BORDER_REFLECT_101 where the tile leaves it (an image smaller than the tile: any distance, so the general form).  A tile whose
// entry does not check out is written as zeros.
template <int C>
__global__ __launch_bounds__(256) void tile_norm_kernel(const uint8_t* __restrict__ src, size_t src_bytes, const ImageDesc* __restrict__ descs,
                                                        int num_images, const TileDesc* __restrict__ tiles, int T_h, int T_w, int row_blocks,
                                                        PreArgs pa, float* __restrict__ out) {
  const int k = blockIdx.x / row_blocks, y_begin = (blockIdx.x % row_blocks) * kTileRowsPerBlock;
  const int y_end = min(y_begin + kTileRowsPerBlock, T_h);
  const TileDesc t = tiles[k];
  bool ok = t.image >= 0 && t.image < num_images && t.y0 >= 0 && t.x0 >= 0;      // (uniform over the workgroup)
  ImageDesc d; d.offset = 0; d.h = 1; d.w = 1;
  if (ok) {
    d = descs[t.image];
    ok = region_ok(d, C, src_bytes) && t.y0 < d.h && t.x0 < d.w;      // sides <= 2^30: origin + tile coordinate stays an int
  }
  for (int y = y_begin; y < y_end; ++y) {
    float* o = out + ((size_t)k * T_h + y) * T_w * 4;
    if (!ok) {
      for (int x = threadIdx.x; x < T_w; x += blockDim.x) { f4 z; z.x = z.y = z.z = z.w = 0.f; *(f4*)(o + (size_t)x * 4) = z; }
      continue;
    }
    const uint8_t* row = src + (size_t)d.offset + (size_t)reflect101(t.y0 + y, d.h) * (size_t)d.w * C;
    for (int x = threadIdx.x; x < T_w; x += blockDim.x) {
      const uint8_t* p = row + (size_t)reflect101(t.x0 + x, d.w) * C;
      f4 v; v.x = 0.f; v.y = 0.f; v.z = 0.f; v.w = 0.f;
      v.x = pre_norm(p[0], pa.mul[0], pa.add[0]);
      if (C > 1) v.y = pre_norm(p[1], pa.mul[1], pa.add[1]);
      if (C > 2) v.z = pre_norm(p[2], pa.mul[2], pa.add[2]);
      if (C > 3) v.w = pre_norm(p[3], pa.mul[3], pa.add[3]);
      __builtin_nontemporal_store(v, (f4*)(o + (size_t)x * 4));
    }
  }
}

hipError_t launch_tile_norm_u8_nhwc4(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int num_images, const TileDesc* tiles, int K,
                                     int C, int T_h, int T_w, const float* mean, const float* std, float* out, hipStream_t st) {
  if (!src || !descs || !tiles || !mean || !std || !out || src_bytes < 1 || num_images < 1 || K < 1 || C < 1 || C > 4 || T_h < 1 || T_w < 1 ||
      T_h > kTileMaxSide || T_w > kTileMaxSide || ((uintptr_t)descs & 7) || ((uintptr_t)tiles & 3) || ((uintptr_t)out & 15))
    return hipErrorInvalidValue;
  const int row_blocks = (T_h + kTileRowsPerBlock - 1) / kTileRowsPerBlock;
  if ((long long)row_blocks * K > 2147483647ll) return hipErrorInvalidValue;
  const PreArgs pa = make_pre_args(C, mean, std);
  const dim3 grid((unsigned)(row_blocks * K)), block(256);
  switch (C) {
    case 1: hipLaunchKernelGGL(tile_norm_kernel<1>, grid, block, 0, st, src, src_bytes, descs, num_images, tiles, T_h, T_w, row_blocks, pa, out); break;
    case 2: hipLaunchKernelGGL(tile_norm_kernel<2>, grid, block, 0, st, src, src_bytes, descs, num_images, tiles, T_h, T_w, row_blocks, pa, out); break;
    case 3: hipLaunchKernelGGL(tile_norm_kernel<3>, grid, block, 0, st, src, src_bytes, descs, num_images, tiles, T_h, T_w, row_blocks, pa, out); break;
    default: hipLaunchKernelGGL(tile_norm_kernel<4>, grid, block, 0, st, src, src_bytes, descs, num_images, tiles, T_h, T_w, row_blocks, pa, out); break;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------- the forward's logit planes -> the dense tile-logit store
// channel 0 of [npix][ld] -> [npix]: a copy, grid-strided
__global__ __launch_bounds__(256) void tile_store_kernel(const float* __restrict__ logits, int ld, size_t npix, float* __restrict__ store) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) store[i] = logits[i * ld];
}
hipError_t launch_tile_store(const float* logits, int ld, size_t npix, float* store, hipStream_t st) {
  if (!logits || !store || ld < 1 || npix < 1) return hipErrorInvalidValue;
  const size_t blocks = (npix + 255) / 256;
  hipLaunchKernelGGL(tile_store_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, logits, ld, npix, store);
  return hipGetLastError();
}

// ---------------------------------------------------------------- the blend: tile logits -> one plane per image, thresholded
// kTileBlendBlocks workgroups per image walk its H_i x W_i pixels with a grid stride.  Pixel (Y, X) finds the tiles that cover it
// from the plan's arithmetic (axis_cover), in ascending (jy, jx) order.  Under one tile it takes that tile's logit unchanged;
// otherwise acc = w_0 * l_0, acc += w_k * l_k, v = acc / sum(w), every operation rounded to float32 on its own (no contraction),
// with the integer weights w = wy * wx of axis_weight (exact in float32, and so is their sum, for tile sides <= 1024).
// An image whose mask region does not fit [0, mask_bytes) is skipped; one whose plan or input descriptor does not check out gets
// zeros.  No entry of the tile table is read here: the store index follows from (first, jy, jx), which the checks bound by K.
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ store, int K, const TileImage* __restrict__ plans, int T_h, int T_w,
                                                         int overlap, const ImageDesc* __restrict__ in_descs, size_t src_bytes, int C,
                                                         const ImageDesc* __restrict__ out_descs, float thr, int apply_sigmoid,
                                                         uint8_t* __restrict__ mask, size_t mask_bytes, float* __restrict__ logits_out) {
#pragma clang fp contract(off)
  const int n = blockIdx.x / kTileBlendBlocks, blk = blockIdx.x % kTileBlendBlocks;
  const ImageDesc d = out_descs[n];
  if (!region_ok(d, 1, mask_bytes)) return;
  const int H = d.h, W = d.w;
  const int Sy = T_h - overlap, Sx = T_w - overlap;
  const int ny = axis_tiles(H, T_h, Sy), nx = axis_tiles(W, T_w, Sx);
  const TileImage p = plans[n];
  bool ok = p.ny == ny && p.nx == nx && p.first >= 0 && (long long)ny * nx <= (long long)K - p.first;
  if (ok && in_descs) {                                  // the image the tiles were cut from: one that gave zero tiles gives a zero mask
    const ImageDesc s = in_descs[n];
    ok = s.h == H && s.w == W && region_ok(s, C, src_bytes);
  }
  uint8_t* out = mask + d.offset;
  float* lo = logits_out ? logits_out + d.offset : nullptr;
  const size_t total = (size_t)H * W, plane = (size_t)T_h * T_w;
  const float* base = store + (ok ? (size_t)p.first * plane : 0);
  for (size_t i = blk * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)kTileBlendBlocks * blockDim.x) {
    if (!ok) {
      out[i] = 0;
      if (lo) lo[i] = 0.f;
      continue;
    }
    const int X = (int)(i % W), Y = (int)(i / W);
    int jy0, jy1, jx0, jx1;
    axis_cover(Y, ny, H, T_h, Sy, jy0, jy1);
    axis_cover(X, nx, W, T_w, Sx, jx0, jx1);
    float v;
    if (jy0 == jy1 && jx0 == jx1) {
      const int ty = Y - axis_origin(jy0, ny, H, T_h, Sy), tx = X - axis_origin(jx0, nx, W, T_w, Sx);
      v = base[(size_t)(jy0 * nx + jx0) * plane + (size_t)ty * T_w + tx];
    } else {
      float acc = 0.f;
      int wsum = 0;
      bool first = true;
      for (int jy = jy0; jy <= jy1; ++jy) {
        const int ty = Y - axis_origin(jy, ny, H, T_h, Sy), wy = axis_weight(ty, T_h);
        for (int jx = jx0; jx <= jx1; ++jx) {
          const int tx = X - axis_origin(jx, nx, W, T_w, Sx), w = wy * axis_weight(tx, T_w);
          const float t = mul_rn((float)w, base[(size_t)(jy * nx + jx) * plane + (size_t)ty * T_w + tx]);
          acc = first ? t : add_rn(acc, t);
          first = false;
          wsum += w;
        }
      }
      v = div_rn(acc, (float)wsum);
    }
    if (lo) lo[i] = v;
    if (apply_sigmoid) v = 1.f / (1.f + expf(-v));
    out[i] = v > thr ? 255 : 0;
  }
}

hipError_t launch_tile_blend_threshold_ragged(const float* store, int K, const TileImage* plans, int num_images, int T_h, int T_w, int overlap,
                                              const ImageDesc* in_descs, size_t src_bytes, int C, const ImageDesc* out_descs, float thr,
                                              int apply_sigmoid, uint8_t* mask, size_t mask_bytes, float* logits_out, hipStream_t st) {
  if (!store || !plans || !out_descs || !mask || mask_bytes < 1 || K < 1 || num_images < 1 || T_h < 1 || T_w < 1 || T_h > kTileMaxSide ||
      T_w > kTileMaxSide || overlap < 0 || 2 * overlap > (T_h < T_w ? T_h : T_w) || (in_descs && (C < 1 || C > 4 || ((uintptr_t)in_descs & 7))) ||
      ((uintptr_t)out_descs & 7) || ((uintptr_t)plans & 3) || (long long)num_images * kTileBlendBlocks > 2147483647ll)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)(num_images * kTileBlendBlocks)), dim3(256), 0, st, store, K, plans, T_h, T_w, overlap,
                     in_descs, src_bytes, C, out_descs, thr, apply_sigmoid, mask, mask_bytes, logits_out);
  return hipGetLastError();
}

}  // namespace uwm
