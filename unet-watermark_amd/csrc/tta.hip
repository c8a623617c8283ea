// Test-time augmentation (include/uwm.h): the network sees every image or tile under the views of a set (flips and
// quarter turns, the dihedral group D4), every logit plane is mapped back and the planes are averaged before the threshold.  Two
// kernels: the views of the network input (view_permute_kernel) and the inverse-and-merge of the logits (view_merge_kernel).
//
// Input side.  The existing resize / gather kernels write the base planes of the images (tiles) a chunk of slots touches into a
// staging buffer of at most as many planes as the chunk has slots; view_permute_kernel then writes every slot of the chunk into the
// forward's input.  A view is an isometry of the pixel grid, so a 32 x 32 tile of a slot is a 32 x 32 tile of the base plane: the
// tile goes through LDS, read row by row and written row by row, so that both sides are whole 512-byte runs for the quarter turns too
// (without LDS a wave's contiguous 16-byte stores would each read a line of their own from a column of the base plane).  Chosen over
// a view code inside the resize / gather kernels: those stage source ROWS per output row, which a quarter turn would make columns of,
// and the extra pass is 32 bytes per pixel and slot beside a forward of several hundred kilobytes per pixel.
//
// Merge side.  One thread owns one pixel of one image (tile) and walks the views of that image present in the chunk in slot order:
// the first view of an image writes, later views add, the last divides by k; every operation is rounded to float32 on its own and
// there is no atomic, so the result is fixed by the slot order and not by the chunking.  A workgroup is a 16 x 16 pixel tile: under a
// quarter turn its reads are 16 runs of 16 logits (element stride ld), each run consumed whole by the workgroup, as its rows are
// under the identity, so the cache lines fetched are the same either way.
#include "uwm_kernels.h"

namespace uwm {

typedef float f4 __attribute__((ext_vector_type(4)));

namespace {
#include "image_common.inc"

// pixel (Y, X) of view c = r + 4 f of an H x W plane (H == W for odd r) reads the plane at (y, x):
// view_c(a) = rot90^r(hflip^f(a)), rot90 counter-clockwise: rot90(a)[Y][X] = a[X][W - 1 - Y]
__device__ __forceinline__ void view_src(int c, int H, int W, int Y, int X, int& y, int& x) {
  const int r = c & 3;
  int fy = Y, fx = X;
  if (r == 1) { fy = X; fx = W - 1 - Y; }
  else if (r == 2) { fy = H - 1 - Y; fx = W - 1 - X; }
  else if (r == 3) { fy = H - 1 - X; fx = Y; }
  if (c & 4) fx = W - 1 - fx;
  y = fy; x = fx;
}
// the inverse: pixel (y, x) of the plane is pixel (Y, X) of view c
__device__ __forceinline__ void view_dst(int c, int H, int W, int y, int x, int& Y, int& X) {
  const int r = c & 3;
  const int fx = (c & 4) ? W - 1 - x : x, fy = y;
  Y = fy; X = fx;
  if (r == 1) { Y = W - 1 - fx; X = fy; }
  else if (r == 2) { Y = H - 1 - fy; X = W - 1 - fx; }
  else if (r == 3) { Y = fx; X = H - 1 - fy; }
}
// the j-th set bit of views (0 <= j < popcount)
__device__ __forceinline__ int view_code(int views, int j) {
  int c = 0;
  for (; c < 8; ++c)
    if ((views >> c) & 1) { if (j == 0) break; --j; }
  return c;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float div_rn(float a, float b) {      // IEEE division (hipcc's default: correctly rounded)
#pragma clang fp contract(off)
  return a / b;
}
inline int popcount8(int v) { int k = 0; for (int c = 0; c < 8; ++c) k += (v >> c) & 1; return k; }
inline bool bad_views(int views, int H, int W) { return views < 1 || views > 255 || ((views & 0xAA) && H != W); }
}  // namespace

constexpr int kViewTile = 32;       // side of the input side's LDS tile
constexpr int kMergeTile = 16;      // side of the merge's pixel tile

// ---------------------------------------------------------------- the views of the network input
// out[slot - slot0][Y][X] = stage[item - item0][view_src(Y, X)], item = slot / k, code = the (slot % k)-th of the set; a slot whose
// item is not among the n_stage staged planes (a padding slot) is written as zeros.  One workgroup = one 32 x 32 tile of one slot.
__global__ __launch_bounds__(256) void view_permute_kernel(const f4* __restrict__ stage, int item0, int n_stage, int views, int k, int slot0, int H,
                                                           int W, int tiles_x, int tiles_per_plane, f4* __restrict__ out) {
  __shared__ f4 lds[kViewTile][kViewTile + 1];
  const int local = blockIdx.x / tiles_per_plane, tile = blockIdx.x % tiles_per_plane;
  const int Y0 = (tile / tiles_x) * kViewTile, X0 = (tile % tiles_x) * kViewTile;
  const int th = min(kViewTile, H - Y0), tw = min(kViewTile, W - X0);
  const int s = slot0 + local, li = s / k - item0;
  f4* o = out + (size_t)local * H * W;
  if (li >= n_stage) {                                  // (uniform over the workgroup)
    f4 z; z.x = z.y = z.z = z.w = 0.f;
    for (int i = threadIdx.x; i < th * tw; i += blockDim.x) o[(size_t)(Y0 + i / tw) * W + X0 + i % tw] = z;
    return;
  }
  const int c = view_code(views, s % k);
  int ya, xa, yb, xb;
  view_src(c, H, W, Y0, X0, ya, xa);
  view_src(c, H, W, Y0 + th - 1, X0 + tw - 1, yb, xb);
  const int sy0 = min(ya, yb), sx0 = min(xa, xb), sw = abs(xa - xb) + 1, sh = abs(ya - yb) + 1;      // the same tile in the base plane
  const f4* b = stage + (size_t)li * H * W;
  for (int i = threadIdx.x; i < sh * sw; i += blockDim.x) lds[i / sw][i % sw] = b[(size_t)(sy0 + i / sw) * W + sx0 + i % sw];
  __syncthreads();
  for (int i = threadIdx.x; i < th * tw; i += blockDim.x) {
    const int Y = Y0 + i / tw, X = X0 + i % tw;
    int y, x;
    view_src(c, H, W, Y, X, y, x);
    o[(size_t)Y * W + X] = lds[y - sy0][x - sx0];
  }
}

// slots [slot0, slot0 + num_slots) of the view set -> the items (images / tiles) they touch: first item and how many of them exist
static void slot_items(int views, int slot0, int num_slots, int num_items, int& item0, int& n_stage) {
  const int k = popcount8(views);
  item0 = slot0 / k;
  const int last = (int)std::min<long long>(((long long)slot0 + num_slots - 1) / k, (long long)num_items - 1);
  n_stage = last >= item0 ? last - item0 + 1 : 0;
}
int view_stage_planes(int views, int num_slots) {
  if (views < 1 || views > 255 || num_slots < 1) return 0;
  const int k = popcount8(views);
  return (int)std::min<long long>(num_slots, ((long long)num_slots + k - 2) / k + 1);
}
static bool bad_view_range(int views, int slot0, int num_slots, int num_items, int H, int W) {
  return bad_views(views, H, W) || slot0 < 0 || num_slots < 1 || num_items < 1 || H < 1 || W < 1 ||
         (long long)slot0 + num_slots > 2147483647ll;
}
static hipError_t launch_view_permute(const float* stage, int item0, int n_stage, int views, int slot0, int num_slots, int H, int W, float* out,
                                      hipStream_t st) {
  const int tiles_x = (W + kViewTile - 1) / kViewTile, tiles_y = (H + kViewTile - 1) / kViewTile;
  if ((long long)tiles_x * tiles_y * num_slots > 2147483647ll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(view_permute_kernel, dim3((unsigned)(tiles_x * tiles_y * num_slots)), dim3(256), 0, st, (const f4*)stage, item0, n_stage, views,
                     popcount8(views), slot0, H, W, tiles_x, tiles_x * tiles_y, (f4*)out);
  return hipGetLastError();
}
hipError_t launch_resize_norm_view_u8_nhwc4(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int num_images, int C, int H, int W,
                                            const float* mean, const float* std, int views, int slot0, int num_slots, float* stage, float* out,
                                            hipStream_t st) {
  if (bad_view_range(views, slot0, num_slots, num_images, H, W) || !stage || !out || (((uintptr_t)stage | (uintptr_t)out) & 15))
    return hipErrorInvalidValue;
  int item0, n_stage;
  slot_items(views, slot0, num_slots, num_images, item0, n_stage);
  if (n_stage > 0) UWM_CHK(launch_resize_norm_u8_nhwc4(src, src_bytes, descs + item0, n_stage, C, H, W, mean, std, stage, st));
  return launch_view_permute(stage, item0, n_stage, views, slot0, num_slots, H, W, out, st);
}
hipError_t launch_tile_norm_view_u8_nhwc4(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int num_images, const TileDesc* tiles, int K,
                                          int C, int T_h, int T_w, const float* mean, const float* std, int views, int slot0, int num_slots,
                                          float* stage, float* out, hipStream_t st) {
  if (bad_view_range(views, slot0, num_slots, K, T_h, T_w) || !stage || !out || (((uintptr_t)stage | (uintptr_t)out) & 15))
    return hipErrorInvalidValue;
  int item0, n_stage;
  slot_items(views, slot0, num_slots, K, item0, n_stage);
  if (n_stage > 0) UWM_CHK(launch_tile_norm_u8_nhwc4(src, src_bytes, descs, num_images, tiles + item0, n_stage, C, T_h, T_w, mean, std, stage, st));
  return launch_view_permute(stage, item0, n_stage, views, slot0, num_slots, T_h, T_w, out, st);
}

// ---------------------------------------------------------------- the inverse-and-merge of the logits
// logits: the planes [num_slots][H][W] (element stride ld) of slots slot0 ..; store: one plane [H][W] per item.  Pixel (y, x) of item i
// walks the views j of i whose slot i * k + j lies in the range, in ascending j: acc = (j == 0 ? l' : acc + l'), l' the logit of view
// c_j at view_dst(y, x); where the range starts inside the item, acc starts from the store; after view k - 1, acc / (float)k (k > 1).
__global__ __launch_bounds__(256) void view_merge_kernel(const float* __restrict__ logits, int ld, int H, int W, int views, int k, int slot0,
                                                         int num_slots, int item0, int tiles_x, int tiles_per_plane, float* __restrict__ store) {
#pragma clang fp contract(off)
  const int item = item0 + blockIdx.x / tiles_per_plane, tile = blockIdx.x % tiles_per_plane;
  const int y = (tile / tiles_x) * kMergeTile + threadIdx.x / kMergeTile, x = (tile % tiles_x) * kMergeTile + threadIdx.x % kMergeTile;
  if (y >= H || x >= W) return;
  const long long first = (long long)item * k, end = (long long)slot0 + num_slots;
  const int j_lo = first < slot0 ? (int)(slot0 - first) : 0, j_hi = first + k > end ? (int)(end - first) : k;
  const size_t plane = (size_t)H * W;
  float* p = store + (size_t)item * plane + (size_t)y * W + x;
  float acc = j_lo > 0 ? *p : 0.f;
  int j = 0;
  for (int c = 0; c < 8; ++c) {
    if (!((views >> c) & 1)) continue;
    if (j >= j_lo && j < j_hi) {
      int Y, X;
      view_dst(c, H, W, y, x, Y, X);
      const float v = logits[((size_t)(first + j - slot0) * plane + (size_t)Y * W + X) * ld];
      acc = j == 0 ? v : add_rn(acc, v);
    }
    ++j;
  }
  if (j_hi == k && k > 1) acc = div_rn(acc, (float)k);
  *p = acc;
}
hipError_t launch_view_merge(const float* logits, int ld, int H, int W, int views, int slot0, int num_slots, int num_items, float* store,
                             hipStream_t st) {
  if (bad_view_range(views, slot0, num_slots, num_items, H, W) || !logits || !store || ld < 1) return hipErrorInvalidValue;
  int item0, n_items;
  slot_items(views, slot0, num_slots, num_items, item0, n_items);
  if (n_items < 1) return hipSuccess;                   // padding slots only: their logits are ignored
  const int tiles_x = (W + kMergeTile - 1) / kMergeTile, tiles_y = (H + kMergeTile - 1) / kMergeTile;
  if ((long long)tiles_x * tiles_y * n_items > 2147483647ll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(view_merge_kernel, dim3((unsigned)(tiles_x * tiles_y * n_items)), dim3(256), 0, st, logits, ld, H, W, views, popcount8(views),
                     slot0, num_slots, item0, tiles_x, tiles_x * tiles_y, store);
  return hipGetLastError();
}

}  // namespace uwm
