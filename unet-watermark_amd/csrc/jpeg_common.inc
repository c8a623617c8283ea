// What the two JPEG round trips share (jpeg_u8.hip: one shape, sides multiples of 16; jpeg_ragged_u8.hip: a ragged batch at any size):
// the pass-A workgroup layout, Annex K's tables and libjpeg's integer DCT passes.  Included inside the anonymous namespace of each file
// (after uwm_kernels.h, inside namespace uwm), the way image_common.inc is.  The rule is stated in include/uwm.h; tests/jpeg_ref.py is
// its numpy form and asserts that every operand stays inside int32.

constexpr int kJpegMcus = 4;                 // MCUs of one pass-A workgroup: 4 * 64 quads = 256 threads, 24 blocks = 192 DCT lanes
constexpr int kJpegBlkStride = 72;           // ints between two blocks in LDS (64 + 8: the column reads of four blocks miss each other's banks)

// Annex K, natural (row-major) order
__device__ const unsigned char kJpegLum[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                               14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
__device__ const unsigned char kJpegChrom[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                                 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

__device__ __forceinline__ int jpeg_quality(const int* __restrict__ quality, int n) { return min(max(quality[n], 0), 100); }
__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint's 1-D pass on d[0..7] in place.  kRows: the row pass (outputs scaled up by 4); else the column pass (scaled back down)
template <bool kRows>
__device__ __forceinline__ void jpeg_fdct_1d(int* d) {
  constexpr int n = kRows ? 11 : 15;
  int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (kRows) { d[0] = (t10 + t11) << 2; d[4] = (t10 - t11) << 2; }
  else { d[0] = jpeg_descale(t10 + t11, 2); d[4] = jpeg_descale(t10 - t11, 2); }
  int z1 = (t12 + t13) * 4433;
  d[2] = jpeg_descale(z1 + t13 * 6270, n);
  d[6] = jpeg_descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  d[7] = jpeg_descale(t4 + z1 + z3, n);
  d[5] = jpeg_descale(t5 + z2 + z4, n);
  d[3] = jpeg_descale(t6 + z2 + z3, n);
  d[1] = jpeg_descale(t7 + z1 + z4, n);
}

// jidctint's 1-D pass on d[0..7] in place.  kCols: the column pass, D(., 11); else the row pass, D(., 18)
template <bool kCols>
__device__ __forceinline__ void jpeg_idct_1d(int* d) {
  constexpr int n = kCols ? 11 : 18;
  int z2 = d[2], z3 = d[6];
  int z1 = (z2 + z3) * 4433;
  int t2 = z1 - z3 * 15137, t3 = z1 + z2 * 6270;
  int t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = d[7]; t1 = d[5]; t2 = d[3]; t3 = d[1];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  d[0] = jpeg_descale(t10 + t3, n); d[7] = jpeg_descale(t10 - t3, n);
  d[1] = jpeg_descale(t11 + t2, n); d[6] = jpeg_descale(t11 - t2, n);
  d[2] = jpeg_descale(t12 + t1, n); d[5] = jpeg_descale(t12 - t1, n);
  d[3] = jpeg_descale(t13 + t0, n); d[4] = jpeg_descale(t13 - t0, n);
}
