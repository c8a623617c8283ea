// Text-watermarked training samples on the device: the text branch of the reference's src/scripts/gen_data.py (apply_text_effects,
// generate_text_watermark, and generate_mixed_watermark's mask rule) executed from host-drawn descriptors.  The host rasterises each
// text to one coverage byte per pixel; everything after that runs here.  The rule is stated in include/uwm.h and DESIGN.md 8o and
// restated in tests/textsynth_ref.py; the stage arithmetic is the logo chain's (synth_stages.inc), integer work or correctly rounded
// IEEE arithmetic (this file is built with -ffp-contract=off), so results are exact and the same on every run.
//
// A job = one text on one image; K slots per image, J = N * K jobs.  Every launch is J * kSynthBlocks workgroups of 256 threads, whatever
// the descriptors hold, so one captured graph serves every batch.  A job's RGBA patch ping-pongs between two buffers of its workspace
// slice: COLOUR writes buffer 0, the c-th stage that runs after it reads buffer (c - 1) & 1 and writes buffer c & 1; a stage that is
// off returns at once.  Every kernel derives the same plan (sizes, which stages run, does it fit) from the descriptor, so a job that
// is disabled or does not fit is skipped by all of them.
#include "uwm_kernels.h"

namespace uwm {

namespace {

#include "image_common.inc"
#include "synth_stages.inc"
#include "synth_chain.inc"

enum { S_COLOUR = 0, S_ROT, S_SCH, S_SCV, S_BLUR0, S_FINISH = S_BLUR0 + 6, S_FIT0, S_END = S_FIT0 + 6 };

// a factor of exactly 1 is Image.blend's copy, so an enhancement step that is off is that step at 1
__device__ __forceinline__ float factor(int on, float f) { return on ? f : 1.f; }

// the text chain's recipe (synth_chain.inc).  COLOUR always runs and fills buffer 0, so every later stage reads a workspace buffer
struct Text {
  typedef TextJob Job;
  enum { kTables = 8, kStages = S_END, kRot = S_ROT, kBlur0 = S_BLUR0, kFinish = S_FINISH };      // tables: scale h, v and three fits h, v
  typedef ChainPlan<kStages, kTables> Plan;
  static constexpr bool kReadsAtlas = false, kSkipsBareImages = true;
  static __device__ __forceinline__ int stage_of(int t) { return t < 2 ? S_SCH + t : S_FIT0 + (t - 2); }
  static __device__ __forceinline__ bool luma_factor(const Job& j, float& fb) { fb = factor(j.brighten, j.brightness); return j.recontrast != 0; }
  static __device__ __forceinline__ int paste_mode(int mask_mode) { return mask_mode; }      // 0: kMaskOver, 1 (the mixed rule): kMaskHalve
  static __device__ bool make_plan(const TextJob& j, const ImageDesc* __restrict__ plane_descs, int num_planes, size_t plane_bytes, int P, int T, Plan& p);
  static hipError_t launch_stages(const Args<Text>& a, hipStream_t st);
};

// the one place that decides whether job j runs: true only if every read and write of every stage stays inside its buffer
__device__ bool Text::make_plan(const TextJob& j, const ImageDesc* __restrict__ plane_descs, int num_planes, size_t plane_bytes, int P, int T, Plan& p) {
  if (!j.enabled || j.glyph < 0 || j.glyph >= num_planes) return false;
  const ImageDesc gd = plane_descs[j.glyph];
  if ((gd.offset & 3) || !region_ok(gd, 1, plane_bytes, 1, kMaxSide)) return false;
  p.off = gd.offset;
  int w = gd.w, h = gd.h;
  plan_clear<Text>(p);
  for (int c = 0; c < 3; ++c) if (j.ink[c] < 0 || j.ink[c] > 255) return false;
  p.w[S_COLOUR] = w; p.h[S_COLOUR] = h;
  if (!patch_fits(w, h, P)) return false;
  p.run[S_COLOUR] = true;
  if (!plan_rotate<Text>(p, w, h, j, P)) return false;
  if (!plan_resize<Text>(p, w, h, S_SCH, j.scale != 0, j.w3, j.h3, P, T)) return false;
  if (!plan_blur<Text>(p, j)) return false;
  for (int s = S_BLUR0; s <= S_FINISH; ++s) { p.w[s] = w; p.h[s] = h; }
  p.run[S_FINISH] = true;
  if (j.nfit < 0 || j.nfit > 3) return false;
  for (int f = 0; f < 3; ++f)
    if (!plan_resize<Text>(p, w, h, S_FIT0 + 2 * f, f < j.nfit, j.fit[f][0], j.fit[f][1], P, T)) return false;
  p.w[S_END] = w; p.h[S_END] = h;
  if (!place_ok(j.x, j.y)) return false;
  plan_count<Text>(p);
  return true;
}

// stage A: what ImageDraw.text leaves on a transparent canvas
__global__ __launch_bounds__(256) void text_colour_kernel(Args<Text> a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const TextJob& j = a.jobs[job];
  Text::Plan p;
  if (!plan_of(a, job, p)) return;
  const uint8_t* __restrict__ cov = a.src + p.off;
  uint32_t* __restrict__ dst = slice_of(a, job).buf[0];
  const uint32_t ink = pack4(j.ink[0], j.ink[1], j.ink[2], 0);
  const int total = p.w[S_COLOUR] * p.h[S_COLOUR];
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const uint32_t c = cov[i];
    dst[i] = c ? ink | (c << 24) : 0u;
  }
}

// stages E - G: Brightness, Contrast, opacity
__global__ __launch_bounds__(256) void text_finish_kernel(Args<Text> a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const TextJob& j = a.jobs[job];
  Text::Plan p;
  if (!plan_of(a, job, p)) return;
  const auto sl = slice_of(a, job);
  const uint32_t* __restrict__ src = stage_src(a, p, sl, S_FINISH);
  uint32_t* __restrict__ dst = stage_dst<Text>(p, sl, S_FINISH);
  const int total = p.w[S_FINISH] * p.h[S_FINISH];
  const int mean = j.recontrast ? luma_mean(sl.part, total) : 0;
  const float fb = factor(j.brighten, j.brightness), fc = factor(j.recontrast, j.contrast);
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const uint32_t v = src[i];
    int r = blend8(0, v & 255, fb), g = blend8(0, (v >> 8) & 255, fb), b = blend8(0, (v >> 16) & 255, fb);
    r = blend8(mean, r, fc); g = blend8(mean, g, fc); b = blend8(mean, b, fc);
    dst[i] = pack4(r, g, b, j.opacity[v >> 24]);
  }
}

// 19 launches: tables, COLOUR, ROTATE, 2 SCALE passes, 6 BLUR passes, the Contrast mean, ENHANCE + OPACITY, 6 FIT passes
hipError_t Text::launch_stages(const Args<Text>& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.J * kB)), block(256);
  hipLaunchKernelGGL(chain_tables_kernel<Text>, grid, block, 0, st, a);
  hipLaunchKernelGGL(text_colour_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(chain_rotate_kernel<Text>, grid, block, 0, st, a);
  hipLaunchKernelGGL(chain_resample_kernel<Text>, grid, block, 0, st, a, (int)S_SCH);
  hipLaunchKernelGGL(chain_resample_kernel<Text>, grid, block, 0, st, a, (int)S_SCV);
  for (int pass = 0; pass < 6; ++pass) hipLaunchKernelGGL(chain_blur_kernel<Text>, grid, block, 0, st, a, pass);
  hipLaunchKernelGGL(chain_luma_kernel<Text>, grid, block, 0, st, a);
  hipLaunchKernelGGL(text_finish_kernel, grid, block, 0, st, a);
  for (int s = S_FIT0; s < S_END; ++s) hipLaunchKernelGGL(chain_resample_kernel<Text>, grid, block, 0, st, a, s);
  return hipGetLastError();
}

}  // namespace

size_t synth_text_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps) {
  return chain_workspace_bytes<Text>(N, K, max_patch_pixels, max_taps);
}

hipError_t launch_synth_text_u8(uint8_t* images, size_t image_bytes, const ImageDesc* image_descs, uint8_t* masks, size_t mask_bytes,
                                const ImageDesc* mask_descs, int mask_mode, const uint8_t* planes, size_t plane_bytes,
                                const ImageDesc* plane_descs, int num_planes, const TextJob* jobs, int N, int K, long long P, long long T,
                                void* ws, size_t ws_bytes, hipStream_t st) {
  if (mask_mode != kMaskOver && mask_mode != kMaskHalve) return hipErrorInvalidValue;
  return launch_chain_batch<Text>(images, image_bytes, image_descs, masks, mask_bytes, mask_descs, mask_mode, planes, plane_bytes, plane_descs,
                                  num_planes, jobs, N, K, P, T, ws, ws_bytes, st);
}

hipError_t launch_text_patches(const uint8_t* planes, size_t plane_bytes, const ImageDesc* plane_descs, int num_planes, const TextJob* jobs, int J,
                               long long P, long long T, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, hipStream_t st) {
  return launch_chain_patches<Text>(planes, plane_bytes, plane_descs, num_planes, jobs, J, P, T, ws, ws_bytes, out, out_bytes, st);
}

}  // namespace uwm
