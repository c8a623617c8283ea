// The JPEG quality-95 save of the reference's gen_data.py (gen_data.py:908; the temporary file of a mixed sample, gen_data.py:402-410)
// on the device: what a baseline 4:2:0 JPEG encode + decode does to the pixels of every image of a RAGGED batch, each at its own size,
// any h and w >= 1.  The arithmetic is jpeg_u8.hip's (jpeg_common.inc); what is new is libjpeg's edge rule (include/uwm.h, DESIGN.md
// 8q; tests/jpeg_any_ref.py is the numpy form, held to Pillow bit for bit):
//   Y        the last column and row are replicated out to multiples of 8;
//   Cb, Cr   columns are replicated at full resolution, in front of the 2 x 2 down-sampling; rows are replicated behind it (down-sampled
//            row hc - 1 fills the rows below it), an odd last image row being doubled first;
//   back     the triangle filter runs on the cropped hc x wc plane; with wc <= 2 every chroma sample fills its 2 x 2 pixels instead.
//
// Two passes over a workspace of `bytes` bytes that holds image i's cropped planes (Y [h][w], Cb and Cr [hc][wc], uint8) back to
// back at the image's own offset: h*w + 2*hc*wc <= 3*h*w, so the planes of two images never meet and no prefix sum is needed.
//   (A) K workgroups per image, each striding over the image's groups of four 16 x 16 MCUs: jpeg_u8.hip's pass A with clamped reads
//       and guarded plane stores.  It only reads `in`.
//   (B) K workgroups per image, each striding over the image's spans of four pixels of a row: planes -> RGB.  It reads `in` only for
//       an image of quality 0, and only where out != in.
// Geometry and qualities are DEVICE memory and both grids are N * K, K from max_pixels: a captured graph serves every batch of N
// images that fits.  An image whose descriptor does not fit (sides < 1, more than max_pixels pixels, not inside `bytes`) is skipped.
#include "uwm_kernels.h"

namespace uwm {

namespace {

#include "image_common.inc"
#include "jpeg_common.inc"

// the image's descriptor when both passes serve it
__device__ __forceinline__ bool jpeg_ragged_ok(const ImageDesc& d, size_t bytes, long long max_pixels) {
  return region_ok(d, 3, bytes) && (long long)d.h * d.w <= max_pixels;
}

// 8 plane bytes of row `row`, columns col .. col + 7 of a rows x cols plane: one 8-byte store where whole and aligned, else bytes
__device__ __forceinline__ void store_row8(uint8_t* __restrict__ plane, int rows, int cols, int row, int col, uint32_t lo, uint32_t hi) {
  if (row >= rows || col >= cols) return;
  uint8_t* dst = plane + (size_t)row * cols + col;
  if (col + 8 <= cols && ((uintptr_t)dst & 7) == 0) { *(uint2*)dst = make_uint2(lo, hi); return; }
#pragma unroll
  for (int i = 0; i < 8; ++i) if (col + i < cols) dst[i] = (uint8_t)((i < 4 ? lo : hi) >> (8 * (i & 3)));
}

// pass A.  grid = N * K
__global__ __launch_bounds__(256) void jpeg_ragged_blocks_kernel(const uint8_t* __restrict__ in, size_t bytes, const ImageDesc* __restrict__ descs,
                                                                 const int* __restrict__ quality, int K, long long max_pixels,
                                                                 uint8_t* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) int blk[kJpegMcus * 6 * kJpegBlkStride];
  __shared__ int qt[2][64];
  const int n = (int)(blockIdx.x / (unsigned)K), wg = (int)(blockIdx.x - (unsigned)n * (unsigned)K);
  const int q = jpeg_quality(quality, n);
  if (q == 0) return;                                                       // the whole workgroup: pass B copies the input
  const ImageDesc d = descs[n];
  if (!jpeg_ragged_ok(d, bytes, max_pixels)) return;
  const int H = d.h, W = d.w, hc = (H + 1) >> 1, wc = (W + 1) >> 1;
  const uint8_t* img = in + d.offset;
  uint8_t* yp = ws + d.offset;
  uint8_t* cbp = yp + (size_t)H * W;
  uint8_t* crp = cbp + (size_t)hc * wc;
  const int t = threadIdx.x;
  const int mw = (W + 15) >> 4, mcus = mw * ((H + 15) >> 4);                // (H * W < 2^31: mcus fits an int)
  const int groups = (mcus + kJpegMcus - 1) / kJpegMcus;
  if (t < 128) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int base = (t < 64) ? kJpegLum[t] : kJpegChrom[t - 64];
    qt[t >> 6][t & 63] = min(max((base * s + 50) / 100, 1), 255);
  }
  for (int g = wg; g < groups; g += K) {
    {                                                                       // colour conversion and down-sampling: one 2 x 2 quad
      const int m = t >> 6, qy = (t >> 3) & 7, qx = t & 7;
      const int mcu = g * kJpegMcus + m;
      int* mb = blk + m * 6 * kJpegBlkStride;
      int yv[2][2] = {{0, 0}, {0, 0}}, cb = 0, cr = 0;
      if (mcu < mcus) {
        const int my = mcu / mw, mx = mcu - my * mw;
        const int r = my * 8 + qy, c = mx * 8 + qx;                         // the quad's place in the down-sampled plane
        const int ys[2] = {min(2 * r, H - 1), min(2 * r + 1, H - 1)}, xs[2] = {min(2 * c, W - 1), min(2 * c + 1, W - 1)};
        int sb = 0, sr = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const uint8_t* px = img + ((size_t)ys[i] * W + xs[j]) * 3;
            const int rr = px[0], gg = px[1], b = px[2];
            yv[i][j] = ((19595 * rr + 38470 * gg + 7471 * b + 32768) >> 16) - 128;
            sb += (-11059 * rr - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
            sr += (32768 * rr - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
          }
        // chroma rows are replicated BEHIND the down-sampling: a quad below down-sampled row hc - 1 repeats that row's, which for an
        // even H is not what the clamped Y rows gave (H - 2 and H - 1 against H - 1 twice)
        const int rc = min(r, hc - 1);
        const int cys[2] = {2 * rc, min(2 * rc + 1, H - 1)};
        if (cys[0] != ys[0] || cys[1] != ys[1]) {
          sb = 0; sr = 0;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const uint8_t* px = img + ((size_t)cys[i] * W + xs[j]) * 3;
              const int rr = px[0], gg = px[1], b = px[2];
              sb += (-11059 * rr - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
              sr += (32768 * rr - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
            }
        }
        const int bias = 1 + (qx & 1);                                      // (an MCU starts at an even chroma column)
        cb = ((sb + bias) >> 2) - 128;
        cr = ((sr + bias) >> 2) - 128;
      }
      int* yb = mb + ((qy >> 2) * 2 + (qx >> 2)) * kJpegBlkStride + ((2 * qy) & 7) * 8 + ((2 * qx) & 7);
      yb[0] = yv[0][0]; yb[1] = yv[0][1]; yb[8] = yv[1][0]; yb[9] = yv[1][1];
      mb[4 * kJpegBlkStride + qy * 8 + qx] = cb;
      mb[5 * kJpegBlkStride + qy * 8 + qx] = cr;
    }
    __syncthreads();
    const int b = t >> 3, r = t & 7;                                        // block 0..23 (t < 192), row / column 0..7
    const bool dct = t < kJpegMcus * 6 * 8;
    int* bp = blk + (dct ? b : 0) * kJpegBlkStride;                         // (lanes 192..255 only wait at the barriers)
    int dd[8];
    if (dct) {                                                              // fDCT, rows
#pragma unroll
      for (int i = 0; i < 8; ++i) dd[i] = bp[r * 8 + i];
      jpeg_fdct_1d<true>(dd);
#pragma unroll
      for (int i = 0; i < 8; ++i) bp[r * 8 + i] = dd[i];
    }
    __syncthreads();
    if (dct) {                                                              // column r: fDCT, quantise, dequantise, IDCT
#pragma unroll
      for (int i = 0; i < 8; ++i) dd[i] = bp[i * 8 + r];
      jpeg_fdct_1d<false>(dd);
      const int* tab = qt[(b % 6) >= 4 ? 1 : 0];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int qq = tab[i * 8 + r];
        const unsigned qv = (unsigned)qq << 3;
        const int a = (int)(((unsigned)abs(dd[i]) + (qv >> 1)) / qv);       // exact integer division
        dd[i] = (dd[i] < 0 ? -a : a) * qq;
      }
      jpeg_idct_1d<true>(dd);
#pragma unroll
      for (int i = 0; i < 8; ++i) bp[i * 8 + r] = dd[i];
    }
    __syncthreads();
    if (dct) {                                                              // IDCT, rows; + 128, clamp, up to 8 bytes out
#pragma unroll
      for (int i = 0; i < 8; ++i) dd[i] = bp[r * 8 + i];
      jpeg_idct_1d<false>(dd);
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        lo |= (uint32_t)clamp255(dd[i] + 128) << (8 * i);
        hi |= (uint32_t)clamp255(dd[4 + i] + 128) << (8 * i);
      }
      const int m = b / 6, k = b - m * 6;
      const int mcu = g * kJpegMcus + m;
      if (mcu < mcus) {                                                     // only the cropped planes are kept: pass B clamps to them
        const int my = mcu / mw, mx = mcu - my * mw;
        if (k < 4) store_row8(yp, H, W, my * 16 + (k >> 1) * 8 + r, mx * 16 + (k & 1) * 8, lo, hi);
        else store_row8(k == 4 ? cbp : crp, hc, wc, my * 8 + r, mx * 8, lo, hi);
      }
    }
    __syncthreads();                                                        // blk is free for the next group
  }
}

// pass B.  grid = N * K; a span = pixels x .. x + 3 (x a multiple of 4) of one row
__global__ __launch_bounds__(256) void jpeg_ragged_pixels_kernel(const uint8_t* in, uint8_t* out /* may be in */, size_t bytes,
                                                                 const ImageDesc* __restrict__ descs, const int* __restrict__ quality, int K,
                                                                 long long max_pixels, const uint8_t* __restrict__ ws) {
  const int n = (int)(blockIdx.x / (unsigned)K), wg = (int)(blockIdx.x - (unsigned)n * (unsigned)K);
  const ImageDesc d = descs[n];
  if (!jpeg_ragged_ok(d, bytes, max_pixels)) return;
  const int q = jpeg_quality(quality, n);
  if (q == 0 && in == out) return;                                          // the bytes stay
  const int H = d.h, W = d.w, hc = (H + 1) >> 1, wc = (W + 1) >> 1;
  const uint8_t* src = in + d.offset;
  uint8_t* dst = out + d.offset;
  const uint8_t* yp = ws + d.offset;
  const uint8_t* cbp = yp + (size_t)H * W;
  const uint8_t* crp = cbp + (size_t)hc * wc;
  const unsigned w4 = (unsigned)(W + 3) >> 2, spans = w4 * (unsigned)H;     // (<= H * W < 2^31)
  for (unsigned i = (unsigned)wg * 256u + threadIdx.x; i < spans; i += (unsigned)K * 256u) {
    const int y = (int)(i / w4), x = (int)(i - (unsigned)y * w4) * 4;
    const int np = min(4, W - x);                                           // pixels of this span
    const size_t pix = (size_t)y * W + x;
    uint8_t* o = dst + pix * 3;
    const bool whole = np == 4;
    if (q == 0) {                                                           // pass through (out != in)
      const uint8_t* p = src + pix * 3;
      if (whole && (((uintptr_t)p | (uintptr_t)o) & 3) == 0) {
        const uint32_t a = ((const uint32_t*)p)[0], b = ((const uint32_t*)p)[1], c = ((const uint32_t*)p)[2];
        ((uint32_t*)o)[0] = a; ((uint32_t*)o)[1] = b; ((uint32_t*)o)[2] = c;
      } else {
        for (int k = 0; k < np * 3; ++k) o[k] = p[k];
      }
      continue;
    }
    uint32_t yw = 0u;
    {
      const uint8_t* p = yp + pix;
      if (whole && ((uintptr_t)p & 3) == 0) yw = *(const uint32_t*)p;
      else
        for (int k = 0; k < np; ++k) yw |= (uint32_t)p[k] << (8 * k);
    }
    const int r = y >> 1, xc = x >> 1;
    const int x1 = min(xc + 1, wc - 1);
    int ch[2][4];                                                           // up-sampled Cb, Cr minus 128
    if (wc > 2) {                                                           // the triangle filter, clamped to the cropped plane
      const int rn = (y & 1) ? min(r + 1, hc - 1) : max(r - 1, 0);
      const int xs[4] = {max(xc - 1, 0), xc, x1, min(xc + 2, wc - 1)};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const uint8_t* pl = c ? crp : cbp;
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
    } else {                                                                // libjpeg's fall-back: every sample fills its 2 x 2 pixels
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const uint8_t* a = (c ? crp : cbp) + (size_t)r * wc;
        ch[c][0] = ch[c][1] = (int)a[xc] - 128;
        ch[c][2] = ch[c][3] = (int)a[x1] - 128;
      }
    }
    uint32_t wd[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = (int)((yw >> (8 * k)) & 255u), cb = ch[0][k], cr = ch[1][k];
      const int v[3] = {clamp255(yy + ((91881 * cr + 32768) >> 16)), clamp255(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16)),
                        clamp255(yy + ((116130 * cb + 32768) >> 16))};
#pragma unroll
      for (int c = 0; c < 3; ++c) wd[(3 * k + c) >> 2] |= (uint32_t)v[c] << (8 * ((3 * k + c) & 3));
    }
    if (whole && ((uintptr_t)o & 3) == 0) {
      ((uint32_t*)o)[0] = wd[0]; ((uint32_t*)o)[1] = wd[1]; ((uint32_t*)o)[2] = wd[2];
    } else {
      for (int k = 0; k < np * 3; ++k) o[k] = (uint8_t)(wd[k >> 2] >> (8 * (k & 3)));
    }
  }
}

}  // namespace

int jpeg_ragged_blocks_per_image(long long max_pixels) {
  const long long k = (max_pixels + kJpegRaggedPixelsPerBlock - 1) / kJpegRaggedPixelsPerBlock;
  return (int)(k < 1 ? 1 : k > kJpegRaggedMaxBlocks ? kJpegRaggedMaxBlocks : k);
}

hipError_t launch_jpeg_ragged_u8(const uint8_t* in, uint8_t* out, size_t bytes, const ImageDesc* descs, const int* quality, int N,
                                 long long max_pixels, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (!in || !out || !descs || !quality || !workspace || bytes < 1 || workspace_bytes < bytes || N < 1 || max_pixels < 1 ||
      max_pixels >= 2147483647ll || (((uintptr_t)in | (uintptr_t)out | (uintptr_t)quality) & 3) || (((uintptr_t)descs | (uintptr_t)workspace) & 7))
    return hipErrorInvalidValue;
  const int K = jpeg_ragged_blocks_per_image(max_pixels);
  if ((long long)N * K > 2147483647ll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jpeg_ragged_blocks_kernel, dim3((unsigned)(N * K)), dim3(256), 0, st, in, bytes, descs, quality, K, max_pixels,
                     (uint8_t*)workspace);
  hipLaunchKernelGGL(jpeg_ragged_pixels_kernel, dim3((unsigned)(N * K)), dim3(256), 0, st, in, out, bytes, descs, quality, K, max_pixels,
                     (const uint8_t*)workspace);
  return hipGetLastError();
}

}  // namespace uwm
