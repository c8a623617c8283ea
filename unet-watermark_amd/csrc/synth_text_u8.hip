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

#include "synth_stages.inc"

constexpr int kTables = 8;                 // scale h, v and three fits h, v
enum { S_COLOUR = 0, S_ROT, S_SCH, S_SCV, S_BLUR0, S_FINISH = S_BLUR0 + 6, S_FIT0, S_END = S_FIT0 + 6 };

struct Plan {
  long long goff;                          // the coverage plane's byte offset
  int w[S_END + 1], h[S_END + 1];          // size in front of stage s; [S_END] = the finished patch
  int before[S_END + 1];                   // stages that ran in front of stage s
  bool run[S_END];
  int ks[kTables];                         // taps per output of the LANCZOS tables
};

// the table of a resample stage, -1 for any other stage
__device__ __forceinline__ int table_of(int s) { return s == S_SCH ? 0 : s == S_SCV ? 1 : s >= S_FIT0 && s < S_END ? 2 + (s - S_FIT0) : -1; }

// the one place that decides whether job j runs: true only if every read and write of every stage stays inside its buffer
__device__ bool make_plan(const TextJob& j, const ImageDesc* __restrict__ plane_descs, int num_planes, size_t plane_bytes, int P, int T, Plan& p) {
  if (!j.enabled || j.glyph < 0 || j.glyph >= num_planes) return false;
  const ImageDesc gd = plane_descs[j.glyph];
  if (gd.h < 1 || gd.w < 1 || gd.h > kMaxSide || gd.w > kMaxSide || gd.offset < 0 || (gd.offset & 3) || (unsigned long long)gd.offset > plane_bytes ||
      (unsigned long long)gd.h * gd.w > plane_bytes - (unsigned long long)gd.offset)
    return false;
  p.goff = gd.offset;
  int w = gd.w, h = gd.h;
  auto side_ok = [](int v) { return v >= 1 && v <= kMaxSide; };
  auto fits = [P](int a, int b) { return (long long)a * b <= (long long)P; };
  auto table_ok = [T](int in, int out, int& ks) { ks = lanczos_ksize(in, out); return (long long)out * (ks + 2) <= (long long)T; };
  // one Image.resize((tw, th), LANCZOS) in front of stages sh (horizontal pass) and sh + 1 (vertical); an equal side has no pass
  auto resize = [&](int sh, int tw, int th) {
    if (!side_ok(tw) || !side_ok(th)) return false;
    p.w[sh] = w; p.h[sh] = h;
    if (tw != w) { p.run[sh] = true; if (!fits(tw, h) || !table_ok(w, tw, p.ks[table_of(sh)])) return false; w = tw; }
    p.w[sh + 1] = w; p.h[sh + 1] = h;
    if (th != h) { p.run[sh + 1] = true; if (!fits(w, th) || !table_ok(h, th, p.ks[table_of(sh + 1)])) return false; h = th; }
    return true;
  };
  for (int s = 0; s < S_END; ++s) p.run[s] = false;
  for (int t = 0; t < kTables; ++t) p.ks[t] = 0;
  for (int c = 0; c < 3; ++c) if (j.ink[c] < 0 || j.ink[c] > 255) return false;
  p.w[S_COLOUR] = w; p.h[S_COLOUR] = h;
  if (!fits(w, h)) return false;
  p.run[S_COLOUR] = true;
  p.w[S_ROT] = w; p.h[S_ROT] = h;
  if (j.rotate) {
    if (!side_ok(j.w2) || !side_ok(j.h2) || !fits(j.w2, j.h2)) return false;
    for (int i = 0; i < 6; ++i) if (!finite_small(j.rot[i])) return false;
    p.run[S_ROT] = true; w = j.w2; h = j.h2;
  }
  if (j.scale) { if (!resize(S_SCH, j.w3, j.h3)) return false; }
  else { p.w[S_SCH] = p.w[S_SCV] = w; p.h[S_SCH] = p.h[S_SCV] = h; }
  if (j.blur) {
    if (j.blur_r < 0 || j.blur_r > kMaxBlurR) return false;
    for (int s = 0; s < 6; ++s) p.run[S_BLUR0 + s] = true;
  }
  for (int s = S_BLUR0; s <= S_FINISH; ++s) { p.w[s] = w; p.h[s] = h; }
  p.run[S_FINISH] = true;
  if (j.nfit < 0 || j.nfit > 3) return false;
  for (int f = 0; f < 3; ++f) {
    const int sh = S_FIT0 + 2 * f;
    if (f < j.nfit) { if (!resize(sh, j.fit[f][0], j.fit[f][1])) return false; }
    else { p.w[sh] = p.w[sh + 1] = w; p.h[sh] = p.h[sh + 1] = h; }
  }
  p.w[S_END] = w; p.h[S_END] = h;
  if (j.x < -(1 << 30) || j.x > (1 << 30) || j.y < -(1 << 30) || j.y > (1 << 30)) return false;
  int c = 0;
  for (int s = 0; s <= S_END; ++s) { p.before[s] = c; if (s < S_END && p.run[s]) ++c; }
  return true;
}

// the workspace slice of one job: two patch buffers, the tables, the luma partial sums
struct Slice { uint32_t* buf[2]; int* tab[kTables]; long long* part; };
__host__ __device__ __forceinline__ size_t slice_bytes(long long P, long long T) { return (size_t)8 * P + (size_t)4 * kTables * T + (size_t)8 * kSynthBlocks; }
__device__ __forceinline__ Slice slice_of(void* ws, int job, int P, int T) {
  uint8_t* b = (uint8_t*)ws + (size_t)job * slice_bytes(P, T);
  Slice s;
  s.buf[0] = (uint32_t*)b; s.buf[1] = (uint32_t*)(b + (size_t)4 * P);
  for (int t = 0; t < kTables; ++t) s.tab[t] = (int*)(b + (size_t)8 * P + (size_t)4 * T * t);
  s.part = (long long*)(b + (size_t)8 * P + (size_t)4 * kTables * T);
  return s;
}
// (COLOUR always runs, so every later stage has before >= 1 and reads a workspace buffer)
__device__ __forceinline__ const uint32_t* stage_src(const Plan& p, const Slice& sl, int s) { return sl.buf[(p.before[s] - 1) & 1]; }
__device__ __forceinline__ uint32_t* stage_dst(const Plan& p, const Slice& sl, int s) { return sl.buf[p.before[s] & 1]; }
__device__ __forceinline__ const uint32_t* finished(const Plan& p, const Slice& sl) { return sl.buf[(p.before[S_END] - 1) & 1]; }

struct Args {
  const uint8_t* planes; size_t plane_bytes; const ImageDesc* plane_descs; int num_planes;
  const TextJob* jobs; int J, P, T; void* ws;
};
#define TEXT_PLAN(a, job, p) make_plan((a).jobs[job], (a).plane_descs, (a).num_planes, (a).plane_bytes, (a).P, (a).T, p)

__global__ __launch_bounds__(256) void text_tables_kernel(Args a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  Plan p;
  if (!TEXT_PLAN(a, job, p)) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  for (int s = 0; s < S_END; ++s) {
    const int t = table_of(s);
    if (t < 0 || !p.run[s]) continue;
    const bool horiz = !(t & 1);
    lanczos_rows(horiz ? p.w[s] : p.h[s], horiz ? p.w[s + 1] : p.h[s + 1], p.ks[t], sl.tab[t], blk);
  }
}

// stage A: what ImageDraw.text leaves on a transparent canvas
__global__ __launch_bounds__(256) void text_colour_kernel(Args a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const TextJob& j = a.jobs[job];
  Plan p;
  if (!TEXT_PLAN(a, job, p)) return;
  const uint8_t* __restrict__ cov = a.planes + p.goff;
  uint32_t* __restrict__ dst = slice_of(a.ws, job, a.P, a.T).buf[0];
  const uint32_t ink = pack4(j.ink[0], j.ink[1], j.ink[2], 0);
  const int total = p.w[S_COLOUR] * p.h[S_COLOUR];
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const uint32_t c = cov[i];
    dst[i] = c ? ink | (c << 24) : 0u;
  }
}

__global__ __launch_bounds__(256) void text_rotate_kernel(Args a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  Plan p;
  if (!TEXT_PLAN(a, job, p) || !p.run[S_ROT]) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  rotate_pass(stage_src(p, sl, S_ROT), stage_dst(p, sl, S_ROT), p.w[S_ROT], p.h[S_ROT], p.w[S_ROT + 1], p.h[S_ROT + 1], a.jobs[job].rot, blk);
}

// one pass of the SCALE resize or of a FIT resize
__global__ __launch_bounds__(256) void text_resample_kernel(Args a, int s) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  Plan p;
  if (!TEXT_PLAN(a, job, p) || !p.run[s]) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const int t = table_of(s);
  const bool horiz = !(t & 1);
  const bool premul = horiz || !p.run[s - 1];          // the first pass of this resize that runs
  const bool unpremul = !horiz || !p.run[s + 1];       // the last one
  resample_pass(stage_src(p, sl, s), stage_dst(p, sl, s), p.w[s], p.w[s + 1], p.h[s + 1], sl.tab[t], p.ks[t], horiz, premul, unpremul, blk);
}

__global__ __launch_bounds__(256) void text_blur_kernel(Args a, int pass) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const TextJob& j = a.jobs[job];
  const int s = S_BLUR0 + pass;
  Plan p;
  if (!TEXT_PLAN(a, job, p) || !p.run[s]) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  blur_pass(stage_src(p, sl, s), stage_dst(p, sl, s), p.w[s], p.h[s], j.blur_r, j.blur_ww, j.blur_fw, pass < 3, blk);
}

// stages E and F.  A factor of exactly 1 is Image.blend's copy, so a step that is off is that step at 1
__device__ __forceinline__ float factor(int on, float f) { return on ? f : 1.f; }

__global__ __launch_bounds__(256) void text_luma_kernel(Args a) {
  __shared__ long long red[256];
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const TextJob& j = a.jobs[job];
  Plan p;
  if (!TEXT_PLAN(a, job, p) || !j.recontrast) return;      // uniform over the workgroup
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  luma_partial(stage_src(p, sl, S_FINISH), p.w[S_FINISH] * p.h[S_FINISH], factor(j.brighten, j.brightness), blk, red, sl.part + blk);
}

__global__ __launch_bounds__(256) void text_finish_kernel(Args a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const TextJob& j = a.jobs[job];
  Plan p;
  if (!TEXT_PLAN(a, job, p)) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const uint32_t* __restrict__ src = stage_src(p, sl, S_FINISH);
  uint32_t* __restrict__ dst = stage_dst(p, sl, S_FINISH);
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

// stage H: paste, one thread per IMAGE pixel.  A pixel's thread applies the slots that cover it in slot order, so overlapping texts
// need no ordering between workgroups, and it halves its own mask byte, so the halving happens once whatever K is.
__global__ __launch_bounds__(256) void text_paste_kernel(Args a, int K, uint8_t* __restrict__ images, size_t image_bytes, const ImageDesc* __restrict__ image_descs,
                                                         uint8_t* __restrict__ masks, size_t mask_bytes, const ImageDesc* __restrict__ mask_descs, int mask_mode) {
  __shared__ const uint32_t* patch[kSynthMaxSlots];
  __shared__ int px[kSynthMaxSlots], py[kSynthMaxSlots], pw[kSynthMaxSlots], ph[kSynthMaxSlots];
  const int per = K * kB, n = blockIdx.x / per, blk = blockIdx.x % per;
  if ((int)threadIdx.x < K) {
    const int job = n * K + threadIdx.x;
    Plan p;
    pw[threadIdx.x] = 0;
    if (TEXT_PLAN(a, job, p)) {
      patch[threadIdx.x] = finished(p, slice_of(a.ws, job, a.P, a.T));
      px[threadIdx.x] = a.jobs[job].x; py[threadIdx.x] = a.jobs[job].y; pw[threadIdx.x] = p.w[S_END]; ph[threadIdx.x] = p.h[S_END];
    }
  }
  __syncthreads();
  bool any = false;
  for (int k = 0; k < K; ++k) any |= pw[k] != 0;
  if (!any) return;                                    // an image without a text that runs is left as it is, mask included
  const ImageDesc d = image_descs[n];
  if (!rgb_desc_ok(d, image_bytes)) return;
  uint8_t* __restrict__ img = images + d.offset;
  uint8_t* __restrict__ msk = nullptr;
  if (masks) {
    const ImageDesc md = mask_descs[n];
    if (mask_desc_ok(md, d, mask_bytes)) msk = masks + md.offset;
  }
  const int total = d.h * d.w;
  for (int i = blk * 256 + threadIdx.x; i < total; i += per * 256) {
    const int y = i / d.w, x = i - y * d.w;
    int r = 0, g = 0, b = 0;
    int m = (msk && mask_mode == 0) ? msk[i] : 0;      // mode 0 pastes over what the plane holds, mode 1 from 0
    bool loaded = false;
    for (int k = 0; k < K; ++k) {
      const int u = x - px[k], v = y - py[k];
      if (pw[k] == 0 || u < 0 || v < 0 || u >= pw[k] || v >= ph[k]) continue;
      if (!loaded) { r = img[(size_t)3 * i]; g = img[(size_t)3 * i + 1]; b = img[(size_t)3 * i + 2]; loaded = true; }
      const uint32_t s = patch[k][(size_t)v * pw[k] + u];
      const int al = s >> 24;
      r = blend255(s & 255, r, al); g = blend255((s >> 8) & 255, g, al); b = blend255((s >> 16) & 255, b, al);
      m = blend255(al, m, al);
    }
    if (loaded) { img[(size_t)3 * i] = (uint8_t)r; img[(size_t)3 * i + 1] = (uint8_t)g; img[(size_t)3 * i + 2] = (uint8_t)b; }
    if (msk) {
      if (mask_mode != 0) msk[i] = (uint8_t)max((int)msk[i] >> 1, m);
      else if (loaded) msk[i] = (uint8_t)m;
    }
  }
}

// the finished patches, for the stage-level tests: job j's w x h RGBA patch -> out + j * P * 4
__global__ __launch_bounds__(256) void text_export_kernel(Args a, uint32_t* __restrict__ out) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  Plan p;
  if (!TEXT_PLAN(a, job, p)) return;
  const uint32_t* __restrict__ src = finished(p, slice_of(a.ws, job, a.P, a.T));
  const int total = p.w[S_END] * p.h[S_END];
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) out[(size_t)job * a.P + i] = src[i];
}

// 19 launches: tables, COLOUR, ROTATE, 2 SCALE passes, 6 BLUR passes, the Contrast mean, ENHANCE + OPACITY, 6 FIT passes
hipError_t launch_stages(const Args& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.J * kB)), block(256);
  hipLaunchKernelGGL(text_tables_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(text_colour_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(text_rotate_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(text_resample_kernel, grid, block, 0, st, a, (int)S_SCH);
  hipLaunchKernelGGL(text_resample_kernel, grid, block, 0, st, a, (int)S_SCV);
  for (int pass = 0; pass < 6; ++pass) hipLaunchKernelGGL(text_blur_kernel, grid, block, 0, st, a, pass);
  hipLaunchKernelGGL(text_luma_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(text_finish_kernel, grid, block, 0, st, a);
  for (int s = S_FIT0; s < S_END; ++s) hipLaunchKernelGGL(text_resample_kernel, grid, block, 0, st, a, s);
  return hipGetLastError();
}

bool text_args_ok(const uint8_t* planes, size_t plane_bytes, const ImageDesc* plane_descs, int num_planes, const TextJob* jobs, int N, int K,
                  long long P, long long T, void* ws, size_t ws_bytes) {
  const size_t need = synth_text_workspace_bytes(N, K, P, T);
  return planes && plane_descs && jobs && ws && plane_bytes >= 1 && num_planes >= 1 && need != 0 && ws_bytes >= need && !((uintptr_t)planes & 3) &&
         !(((uintptr_t)plane_descs | (uintptr_t)jobs | (uintptr_t)ws) & 7);
}

}  // namespace

size_t synth_text_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps) {
  if (N < 1 || K < 1 || K > kSynthMaxSlots || max_patch_pixels < 1 || max_patch_pixels > kSynthMaxPatchPixels || max_taps < 1 ||
      max_taps > kSynthMaxTaps || (long long)N * K > 2147483647ll / (kB * 4))
    return 0;
  return (size_t)N * K * slice_bytes(max_patch_pixels, max_taps);
}

hipError_t launch_synth_text_u8(uint8_t* images, size_t image_bytes, const ImageDesc* image_descs, uint8_t* masks, size_t mask_bytes,
                                const ImageDesc* mask_descs, int mask_mode, const uint8_t* planes, size_t plane_bytes,
                                const ImageDesc* plane_descs, int num_planes, const TextJob* jobs, int N, int K, long long P, long long T,
                                void* ws, size_t ws_bytes, hipStream_t st) {
  if (!text_args_ok(planes, plane_bytes, plane_descs, num_planes, jobs, N, K, P, T, ws, ws_bytes) || !images || !image_descs || image_bytes < 1 ||
      ((uintptr_t)image_descs & 7) || (masks && (!mask_descs || mask_bytes < 1 || ((uintptr_t)mask_descs & 7))) || (mask_mode != 0 && mask_mode != 1))
    return hipErrorInvalidValue;
  const Args a{planes, plane_bytes, plane_descs, num_planes, jobs, N * K, (int)P, (int)T, ws};
  const hipError_t e = launch_stages(a, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(text_paste_kernel, dim3((unsigned)(N * K * kB)), dim3(256), 0, st, a, K, images, image_bytes, image_descs, masks, mask_bytes,
                     mask_descs, mask_mode);
  return hipGetLastError();
}

hipError_t launch_text_patches(const uint8_t* planes, size_t plane_bytes, const ImageDesc* plane_descs, int num_planes, const TextJob* jobs, int J,
                               long long P, long long T, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, hipStream_t st) {
  if (!text_args_ok(planes, plane_bytes, plane_descs, num_planes, jobs, J, 1, P, T, ws, ws_bytes) || !out || ((uintptr_t)out & 3) ||
      out_bytes / 4 / (size_t)P < (size_t)J)
    return hipErrorInvalidValue;
  const Args a{planes, plane_bytes, plane_descs, num_planes, jobs, J, (int)P, (int)T, ws};
  const hipError_t e = launch_stages(a, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(text_export_kernel, dim3((unsigned)(J * kB)), dim3(256), 0, st, a, (uint32_t*)out);
  return hipGetLastError();
}

}  // namespace uwm
