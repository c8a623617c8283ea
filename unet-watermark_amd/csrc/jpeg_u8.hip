// A.ImageCompression of the reference's transparent_watermark recipe (get_transparent_watermark_transform, src/utils/dataset.py:298-334)
// on the device: what a baseline 4:2:0 JPEG encode + decode does to the pixels of a uint8 RGB image, without the (lossless) entropy
// coding — libjpeg's default path: fixed-point colour conversion, 2 x 2 chroma down-sampling, the "islow" integer DCT, integer
// quantisation, the integer inverse DCT, "fancy" triangle up-sampling, fixed-point colour conversion back, then Normalize.  The rule is
// stated in include/uwm.h and DESIGN.md 8f; it is all int32 work (tests/jpeg_ref.py asserts the operand range), so every result equals
// tests/jpeg_ref.py bit for bit.
//
// Two passes over a workspace of reconstructed planes (Y [N][H][W], Cb and Cr [N][H/2][W/2], uint8):
//   (A) one workgroup per four 16 x 16 MCUs of one image.  A thread converts one 2 x 2 pixel quad (4 Y, one down-sampled Cb, Cr) into
//       the MCU's six 8 x 8 blocks in LDS; then lane = block * 8 + row runs the 1-D passes on eight int32 registers: fDCT rows ->
//       (LDS transpose) -> fDCT columns, quantise, dequantise and the IDCT's column pass, all on the column the lane holds ->
//       (LDS transpose) -> IDCT rows, + 128, clamp, 8 bytes to the plane.  The image's two quality tables are built into LDS.
//   (B) one thread per four output pixels of a row: the chroma triangle filter with its one-sample halo from the planes, colour
//       conversion back, the uint8 image and / or pre_norm.
// An image with quality 0 leaves pass A before any barrier and is copied from the input by pass B.  Both launches are sized from N, H,
// W alone and the qualities are device memory: a captured graph serves every batch of a shape.  The kernels only clamp the quality.
#include "uwm_kernels.h"

namespace uwm {

namespace {
#include "image_common.inc"
#include "jpeg_common.inc"
}  // namespace

// pass A.  grid = N * groups, groups = ceil(MCUs of an image / kJpegMcus)
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const uint8_t* __restrict__ img, const int* __restrict__ quality, int H, int W,
                                                          int groups, uint8_t* __restrict__ yp, uint8_t* __restrict__ cbp,
                                                          uint8_t* __restrict__ crp) {
  __shared__ __attribute__((aligned(16))) int blk[kJpegMcus * 6 * kJpegBlkStride];
  __shared__ int qt[2][64];
  const int n = (int)(blockIdx.x / (unsigned)groups), g = (int)(blockIdx.x - (unsigned)n * (unsigned)groups);
  const int q = jpeg_quality(quality, n);
  if (q == 0) return;                                                       // the whole workgroup: pass B copies the input
  const int t = threadIdx.x;
  const int mw = W >> 4, mcus = mw * (H >> 4);
  if (t < 128) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int base = (t < 64) ? kJpegLum[t] : kJpegChrom[t - 64];
    qt[t >> 6][t & 63] = min(max((base * s + 50) / 100, 1), 255);
  }
  {                                                                         // colour conversion and down-sampling: one 2 x 2 quad
    const int m = t >> 6, qy = (t >> 3) & 7, qx = t & 7;
    const int mcu = g * kJpegMcus + m;
    int* mb = blk + m * 6 * kJpegBlkStride;
    int yv[2][2] = {{0, 0}, {0, 0}}, cb = 0, cr = 0;
    if (mcu < mcus) {
      const int my = mcu / mw, mx = mcu - my * mw;
      const uint8_t* p = img + (((size_t)n * H + my * 16 + 2 * qy) * W + mx * 16 + 2 * qx) * 3;
      int sb = 0, sr = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint8_t* px = p + ((size_t)i * W + j) * 3;
          const int r = px[0], gg = px[1], b = px[2];
          yv[i][j] = ((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16) - 128;
          sb += (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
          sr += (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
        }
      const int bias = 1 + (qx & 1);                                        // (an MCU starts at an even chroma column)
      cb = ((sb + bias) >> 2) - 128;
      cr = ((sr + bias) >> 2) - 128;
    }
    int* yb = mb + ((qy >> 2) * 2 + (qx >> 2)) * kJpegBlkStride + ((2 * qy) & 7) * 8 + ((2 * qx) & 7);
    yb[0] = yv[0][0]; yb[1] = yv[0][1]; yb[8] = yv[1][0]; yb[9] = yv[1][1];
    mb[4 * kJpegBlkStride + qy * 8 + qx] = cb;
    mb[5 * kJpegBlkStride + qy * 8 + qx] = cr;
  }
  __syncthreads();
  const int b = t >> 3, r = t & 7;                                          // block 0..23 (t < 192), row / column 0..7
  const bool dct = t < kJpegMcus * 6 * 8;
  int* bp = blk + (dct ? b : 0) * kJpegBlkStride;                           // (lanes 192..255 only wait at the barriers)
  int d[8];
  if (dct) {                                                                // fDCT, rows
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = bp[r * 8 + i];
    jpeg_fdct_1d<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) bp[r * 8 + i] = d[i];
  }
  __syncthreads();
  if (dct) {                                                                // column r: fDCT, quantise, dequantise, IDCT
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = bp[i * 8 + r];
    jpeg_fdct_1d<false>(d);
    const int* tab = qt[(b % 6) >= 4 ? 1 : 0];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int qq = tab[i * 8 + r];
      const unsigned qv = (unsigned)qq << 3;
      const int a = (int)(((unsigned)abs(d[i]) + (qv >> 1)) / qv);          // exact integer division
      d[i] = (d[i] < 0 ? -a : a) * qq;
    }
    jpeg_idct_1d<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) bp[i * 8 + r] = d[i];
  }
  __syncthreads();
  if (dct) {                                                                // IDCT, rows; + 128, clamp, 8 bytes out
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = bp[r * 8 + i];
    jpeg_idct_1d<false>(d);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      lo |= (uint32_t)clamp255(d[i] + 128) << (8 * i);
      hi |= (uint32_t)clamp255(d[4 + i] + 128) << (8 * i);
    }
    const int m = b / 6, k = b - m * 6;
    const int mcu = g * kJpegMcus + m;
    if (mcu < mcus) {
      const int my = mcu / mw, mx = mcu - my * mw;
      uint8_t* dst;
      if (k < 4) dst = yp + ((size_t)n * H + my * 16 + (k >> 1) * 8 + r) * W + mx * 16 + (k & 1) * 8;
      else dst = (k == 4 ? cbp : crp) + ((size_t)n * (H >> 1) + my * 8 + r) * (W >> 1) + mx * 8;
      *(uint2*)dst = make_uint2(lo, hi);                                    // 8-byte aligned: W % 16 == 0, planes 16-byte aligned
    }
  }
}

// pass B: thread i = ((n * H + y) * (W / 4) + x / 4) makes pixels x .. x + 3 of row y (img and out_u8 4-byte, out_f 16-byte aligned)
__global__ __launch_bounds__(256) void jpeg_pixels_kernel(const uint8_t* __restrict__ img, const int* __restrict__ quality, int H, int W,
                                                          size_t total, PreArgs pa, const uint8_t* __restrict__ yp,
                                                          const uint8_t* __restrict__ cbp, const uint8_t* __restrict__ crp,
                                                          float* __restrict__ out_f, uint8_t* __restrict__ out_u8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int w4 = W >> 2;
  const int x = (int)(i % (size_t)w4) * 4;
  const size_t row = i / (size_t)w4;                                        // n * H + y
  const int y = (int)(row % (size_t)H), n = (int)(row / (size_t)H);
  const size_t pix = row * W + x;
  int v[4][3];
  if (jpeg_quality(quality, n) == 0) {                                      // pass through
    const uint32_t* p4 = (const uint32_t*)(img + pix * 3);
    const uint32_t w0 = p4[0], w1 = p4[1], w2 = p4[2];
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k / 3][k % 3] = (int)(((k < 4 ? w0 : k < 8 ? w1 : w2) >> (8 * (k & 3))) & 255u);
  } else {
    const int hc = H >> 1, wc = W >> 1;
    const int r = y >> 1, rn = (y & 1) ? min(r + 1, hc - 1) : max(r - 1, 0);
    const int xc = x >> 1;
    const int xs[4] = {max(xc - 1, 0), xc, xc + 1, min(xc + 2, wc - 1)};
    const uint32_t yw = *(const uint32_t*)(yp + pix);
    int ch[2][4];                                                           // up-sampled Cb, Cr minus 128
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint8_t* pl = (c ? crp : cbp) + (size_t)n * hc * wc;
      const uint8_t* a = pl + (size_t)r * wc;
      const uint8_t* bb = pl + (size_t)rn * wc;
      int s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = 3 * (int)a[xs[k]] + (int)bb[xs[k]];
      ch[c][0] = ((3 * s[1] + s[0] + 8) >> 4) - 128;
      ch[c][1] = ((3 * s[1] + s[2] + 7) >> 4) - 128;
      ch[c][2] = ((3 * s[2] + s[1] + 8) >> 4) - 128;
      ch[c][3] = ((3 * s[2] + s[3] + 7) >> 4) - 128;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = (int)((yw >> (8 * k)) & 255u), cb = ch[0][k], cr = ch[1][k];
      v[k][0] = clamp255(yy + ((91881 * cr + 32768) >> 16));
      v[k][1] = clamp255(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      v[k][2] = clamp255(yy + ((116130 * cb + 32768) >> 16));
    }
  }
  if (out_u8) {
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) w[k >> 2] |= (uint32_t)v[k / 3][k % 3] << (8 * (k & 3));
    uint32_t* o4 = (uint32_t*)(out_u8 + pix * 3);
    o4[0] = w[0]; o4[1] = w[1]; o4[2] = w[2];
  }
  if (out_f) {
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = out_f + ((size_t)n * 3 + c) * plane + (size_t)y * W + x;
      float f[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) f[k] = pre_norm((uint32_t)v[k][c], pa.mul[c], pa.add[c]);
      *(float4*)o = make_float4(f[0], f[1], f[2], f[3]);
    }
  }
}

size_t jpeg_workspace_bytes(int N, int H, int W) {
  if (N < 1 || H < 16 || W < 16 || (H & 15) || (W & 15)) return 0;
  return (size_t)N * H * W / 2 * 3;                                         // Y + Cb + Cr planes
}

hipError_t launch_jpeg_u8(const uint8_t* img, const int* quality, int N, int H, int W, const float* mean, const float* std, void* workspace,
                          size_t workspace_bytes, float* out_f, uint8_t* out_u8, hipStream_t st) {
  const size_t need = jpeg_workspace_bytes(N, H, W);
  if (!need || !img || !quality || ((uintptr_t)quality & 3) || !mean || !std || (!out_f && !out_u8) || !workspace ||
      ((uintptr_t)workspace & 15) || workspace_bytes < need || ((uintptr_t)img & 3) || ((uintptr_t)out_u8 & 3) || ((uintptr_t)out_f & 15))
    return hipErrorInvalidValue;
  const long long mcus = (long long)(H >> 4) * (W >> 4), groups = (mcus + kJpegMcus - 1) / kJpegMcus;
  const size_t total = (size_t)N * H * (W >> 2);
  const size_t blocks_b = (total + 255) / 256;
  if (groups * N > 2147483647ll || blocks_b > 2147483647ull) return hipErrorInvalidValue;
  const size_t npix = (size_t)N * H * W;
  uint8_t* yp = (uint8_t*)workspace;
  uint8_t* cbp = yp + npix;                                                 // (npix is a multiple of 256: both stay 16-byte aligned)
  uint8_t* crp = cbp + npix / 4;
  const PreArgs pa = make_pre_args(3, mean, std);
  hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((unsigned)(groups * N)), dim3(256), 0, st, img, quality, H, W, (int)groups, yp, cbp, crp);
  hipLaunchKernelGGL(jpeg_pixels_kernel, dim3((unsigned)blocks_b), dim3(256), 0, st, img, quality, H, W, total, pa, (const uint8_t*)yp,
                     (const uint8_t*)cbp, (const uint8_t*)crp, out_f, out_u8);
  return hipGetLastError();
}

}  // namespace uwm
