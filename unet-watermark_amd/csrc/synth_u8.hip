// Logo-watermarked training samples on the device: the logo branch of the reference's src/scripts/gen_data.py (apply_watermark_effects,
// resize_watermark, generate_multiple_watermarks_image) executed from host-drawn descriptors.  The rule is stated in include/uwm.h and
// DESIGN.md 8i and restated in tests/synth_ref.py; every stage is integer work or correctly rounded IEEE arithmetic (this file is built
// with -ffp-contract=off and spells the roundings out), so results are exact and the same on every run.
//
// A job = one logo on one image; K slots per image, J = N * K jobs.  Every launch is J * kSynthBlocks workgroups of 256 threads, whatever
// the descriptors hold, so one captured graph serves every batch.  A job's RGBA patch ping-pongs between two buffers of its workspace
// slice: the c-th stage that runs reads buffer (c - 1) & 1 (the logo itself for c = 0) and writes buffer c & 1; a stage that is off
// returns at once.  Every kernel derives the same plan (sizes, which stages run, does it fit) from the descriptor, so a job that is
// disabled or does not fit is skipped by all of them.
#include "uwm_kernels.h"

namespace uwm {

namespace {

#include "synth_stages.inc"

enum { S_R1H = 0, S_R1V, S_ROT, S_R3H, S_R3V, S_SHEAR, S_BLUR0, S_FINISH = S_BLUR0 + 6, S_END };

struct Plan {
  long long loff;                          // the logo's byte offset
  int w[S_END + 1], h[S_END + 1];          // size in front of stage s; [S_END] = the finished patch
  int before[S_END + 1];                   // stages that ran in front of stage s
  bool run[S_END];
  int ks[4];                               // taps per output of the four LANCZOS tables (r1h, r1v, r3h, r3v)
};

// the one place that decides whether job j runs: true only if every read and write of every stage stays inside its buffer
__device__ bool make_plan(const SynthJob& j, const ImageDesc* __restrict__ logo_descs, int num_logos, size_t logo_bytes, int P, int T, Plan& p) {
  if (!j.enabled || j.logo < 0 || j.logo >= num_logos) return false;
  const ImageDesc ld = logo_descs[j.logo];
  if (ld.h < 1 || ld.w < 1 || ld.h > kMaxSide || ld.w > kMaxSide || ld.offset < 0 || (ld.offset & 3) || (unsigned long long)ld.offset > logo_bytes ||
      (unsigned long long)ld.h * ld.w > (logo_bytes - (unsigned long long)ld.offset) / 4)
    return false;
  p.loff = ld.offset;
  int w = ld.w, h = ld.h;
  auto side_ok = [](int v) { return v >= 1 && v <= kMaxSide; };
  auto fits = [P](int a, int b) { return (long long)a * b <= (long long)P; };
  auto table_ok = [T](int in, int out, int& ks) { ks = lanczos_ksize(in, out); return (long long)out * (ks + 2) <= (long long)T; };
  for (int s = 0; s < S_END; ++s) p.run[s] = false;
  for (int t = 0; t < 4; ++t) p.ks[t] = 0;
  if (!side_ok(j.w1) || !side_ok(j.h1)) return false;
  p.w[S_R1H] = w; p.h[S_R1H] = h;
  if (j.w1 != w) { p.run[S_R1H] = true; if (!fits(j.w1, h) || !table_ok(w, j.w1, p.ks[0])) return false; w = j.w1; }
  p.w[S_R1V] = w; p.h[S_R1V] = h;
  if (j.h1 != h) { p.run[S_R1V] = true; if (!fits(w, j.h1) || !table_ok(h, j.h1, p.ks[1])) return false; h = j.h1; }
  p.w[S_ROT] = w; p.h[S_ROT] = h;
  if (j.rotate) {
    if (!side_ok(j.w2) || !side_ok(j.h2) || !fits(j.w2, j.h2)) return false;
    for (int i = 0; i < 6; ++i) if (!finite_small(j.rot[i])) return false;
    p.run[S_ROT] = true; w = j.w2; h = j.h2;
  }
  p.w[S_R3H] = w; p.h[S_R3H] = h;
  if (j.stretch) {
    if (!side_ok(j.w3) || !side_ok(j.h3)) return false;
    if (j.w3 != w) { p.run[S_R3H] = true; if (!fits(j.w3, h) || !table_ok(w, j.w3, p.ks[2])) return false; w = j.w3; }
  }
  p.w[S_R3V] = w; p.h[S_R3V] = h;
  if (j.stretch && j.h3 != h) { p.run[S_R3V] = true; if (!fits(w, j.h3) || !table_ok(h, j.h3, p.ks[3])) return false; h = j.h3; }
  p.w[S_SHEAR] = w; p.h[S_SHEAR] = h;
  if (j.stretch && j.shear) {
    for (int i = 0; i < 6; ++i) if (!finite_small(j.shear_minv[i])) return false;
    p.run[S_SHEAR] = true;
  }
  if (j.blur) {
    if (j.blur_r < 0 || j.blur_r > kMaxBlurR) return false;
    for (int s = 0; s < 6; ++s) p.run[S_BLUR0 + s] = true;
  }
  for (int s = S_BLUR0; s <= S_END; ++s) { p.w[s] = w; p.h[s] = h; }
  if (!fits(w, h)) return false;                       // (no stage ran: the logo itself must fit the buffer finish writes)
  if (j.ndefects < 0 || j.ndefects > 3) return false;
  for (int d = 0; d < j.ndefects; ++d)
    for (int i = 0; i < 4; ++i) if (j.defects[d][i] < 0 || j.defects[d][i] > kMaxSide) return false;
  if (j.x < -(1 << 30) || j.x > (1 << 30) || j.y < -(1 << 30) || j.y > (1 << 30)) return false;
  p.run[S_FINISH] = true;
  int c = 0;
  for (int s = 0; s <= S_END; ++s) { p.before[s] = c; if (s < S_END && p.run[s]) ++c; }
  return true;
}

// the workspace slice of one job: two patch buffers, four tables, the luma partial sums
struct Slice { uint32_t* buf[2]; int* tab[4]; long long* part; };
__device__ __forceinline__ size_t slice_bytes(int P, int T) { return (size_t)8 * P + (size_t)16 * T + (size_t)8 * kB; }
__device__ __forceinline__ Slice slice_of(void* ws, int job, int P, int T) {
  uint8_t* b = (uint8_t*)ws + (size_t)job * slice_bytes(P, T);
  Slice s;
  s.buf[0] = (uint32_t*)b; s.buf[1] = (uint32_t*)(b + (size_t)4 * P);
  for (int t = 0; t < 4; ++t) s.tab[t] = (int*)(b + (size_t)8 * P + (size_t)4 * T * t);
  s.part = (long long*)(b + (size_t)8 * P + (size_t)16 * T);
  return s;
}
__device__ __forceinline__ const uint32_t* stage_src(const Plan& p, const Slice& sl, const uint8_t* logos, int s) {
  return p.before[s] == 0 ? (const uint32_t*)(logos + p.loff) : sl.buf[(p.before[s] - 1) & 1];
}
__device__ __forceinline__ uint32_t* stage_dst(const Plan& p, const Slice& sl, int s) { return sl.buf[p.before[s] & 1]; }

struct Args {
  const uint8_t* logos; size_t logo_bytes; const ImageDesc* logo_descs; int num_logos;
  const SynthJob* jobs; int J, P, T; void* ws;
};

// ---------------------------------------------------------------------------------------------- LANCZOS tables
__global__ __launch_bounds__(256) void lanczos_table_kernel(int in, int out, int ksize, int* __restrict__ table) {
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx < out) lanczos_row(in, out, ksize, xx, table + (size_t)xx * (ksize + 2));
}

__global__ __launch_bounds__(256) void synth_tables_kernel(Args a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  Plan p;
  if (!make_plan(a.jobs[job], a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p)) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const int stage[4] = {S_R1H, S_R1V, S_R3H, S_R3V};
  for (int t = 0; t < 4; ++t) {
    const int s = stage[t];
    if (!p.run[s]) continue;
    const bool horiz = !(t & 1);
    const int in = horiz ? p.w[s] : p.h[s], out = horiz ? p.w[s + 1] : p.h[s + 1];
    lanczos_rows(in, out, p.ks[t], sl.tab[t], blk);
  }
}

// ---------------------------------------------------------------------------------------------- stages 1 and 3a: one resample pass
__global__ __launch_bounds__(256) void synth_resample_kernel(Args a, int s) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  Plan p;
  if (!make_plan(a.jobs[job], a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p) || !p.run[s]) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const bool horiz = s == S_R1H || s == S_R3H;
  const int t = s == S_R1H ? 0 : s == S_R1V ? 1 : s == S_R3H ? 2 : 3;
  const bool premul = horiz || !p.run[s - 1];          // the first pass of this resize that runs
  const bool unpremul = !horiz || !p.run[s + 1];       // the last one
  const uint32_t* __restrict__ src = stage_src(p, sl, a.logos, s);
  uint32_t* __restrict__ dst = stage_dst(p, sl, s);
  resample_pass(src, dst, p.w[s], p.w[s + 1], p.h[s + 1], sl.tab[t], p.ks[t], horiz, premul, unpremul, blk);
}

// ---------------------------------------------------------------------------------------------- stage 2: Pillow's affine_fixed
__global__ __launch_bounds__(256) void synth_rotate_kernel(Args a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const SynthJob& j = a.jobs[job];
  Plan p;
  if (!make_plan(j, a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p) || !p.run[S_ROT]) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const uint32_t* __restrict__ src = stage_src(p, sl, a.logos, S_ROT);
  uint32_t* __restrict__ dst = stage_dst(p, sl, S_ROT);
  rotate_pass(src, dst, p.w[S_ROT], p.h[S_ROT], p.w[S_ROT + 1], p.h[S_ROT + 1], j.rot, blk);
}

// ---------------------------------------------------------------------------------------------- stage 3b: shear (restated; NOT run against cv2)
__device__ __forceinline__ long long rne1024(double v) { return (long long)rint(__dmul_rn(v, 1024.0)); }

__global__ __launch_bounds__(256) void synth_shear_kernel(Args a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const SynthJob& j = a.jobs[job];
  Plan p;
  if (!make_plan(j, a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p) || !p.run[S_SHEAR]) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const uint32_t* __restrict__ src = stage_src(p, sl, a.logos, S_SHEAR);
  uint32_t* __restrict__ dst = stage_dst(p, sl, S_SHEAR);
  const int w = p.w[S_SHEAR], h = p.h[S_SHEAR];
  const double* m = j.shear_minv;
  const int total = w * h;
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const int y = i / w, x = i - y * w;
    const long long X = (rne1024(__dadd_rn(__dmul_rn(m[1], (double)y), m[2])) + 16 + rne1024(__dmul_rn(m[0], (double)x))) >> 5;
    const long long Y = (rne1024(__dadd_rn(__dmul_rn(m[4], (double)y), m[5])) + 16 + rne1024(__dmul_rn(m[3], (double)x))) >> 5;
    const long long sx = X >> 5, sy = Y >> 5;
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    auto tap = [&](long long yy, long long xx) -> uint32_t { return (xx >= 0 && xx < w && yy >= 0 && yy < h) ? src[(size_t)yy * w + (size_t)xx] : 0u; };
    const uint32_t t00 = tap(sy, sx), t01 = tap(sy, sx + 1), t10 = tap(sy + 1, sx), t11 = tap(sy + 1, sx + 1);
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    uint32_t out = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int sft = 8 * c;
      const int acc = w00 * (int)((t00 >> sft) & 255) + w01 * (int)((t01 >> sft) & 255) + w10 * (int)((t10 >> sft) & 255) + w11 * (int)((t11 >> sft) & 255);
      out |= (uint32_t)((acc + 512) >> 10) << sft;
    }
    dst[i] = out;
  }
}

// ---------------------------------------------------------------------------------------------- stage 4: one extended box blur pass
__global__ __launch_bounds__(256) void synth_blur_kernel(Args a, int pass) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const SynthJob& j = a.jobs[job];
  const int s = S_BLUR0 + pass;
  Plan p;
  if (!make_plan(j, a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p) || !p.run[s]) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const uint32_t* __restrict__ src = stage_src(p, sl, a.logos, s);
  uint32_t* __restrict__ dst = stage_dst(p, sl, s);
  blur_pass(src, dst, p.w[s], p.h[s], j.blur_r, j.blur_ww, j.blur_fw, pass < 3, blk);
}

// ---------------------------------------------------------------------------------------------- stages 5-7
// per-workgroup partial sums of L over the brightened patch (the Contrast degenerate is their mean); integer sums: any order, one result
__global__ __launch_bounds__(256) void synth_luma_kernel(Args a) {
  __shared__ long long red[256];
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const SynthJob& j = a.jobs[job];
  Plan p;
  if (!make_plan(j, a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p) || !j.enhance) return;      // uniform over the workgroup
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const uint32_t* __restrict__ src = stage_src(p, sl, a.logos, S_FINISH);
  luma_partial(src, p.w[S_FINISH] * p.h[S_FINISH], j.brightness, blk, red, sl.part + blk);
}

__global__ __launch_bounds__(256) void synth_finish_kernel(Args a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const SynthJob& j = a.jobs[job];
  Plan p;
  if (!make_plan(j, a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p)) return;
  const Slice sl = slice_of(a.ws, job, a.P, a.T);
  const uint32_t* __restrict__ src = stage_src(p, sl, a.logos, S_FINISH);
  uint32_t* __restrict__ dst = stage_dst(p, sl, S_FINISH);
  const int w = p.w[S_FINISH], total = w * p.h[S_FINISH];
  const int mean = j.enhance ? luma_mean(sl.part, total) : 0;
  const float fb = j.brightness, fc = j.contrast, fs = j.color;
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) {
    const int y = i / w, x = i - y * w;
    const uint32_t v = src[i];
    int r = v & 255, g = (v >> 8) & 255, b = (v >> 16) & 255, al = v >> 24;
    for (int d = 0; d < j.ndefects; ++d)
      if (x >= j.defects[d][0] && x < j.defects[d][0] + j.defects[d][2] && y >= j.defects[d][1] && y < j.defects[d][1] + j.defects[d][3]) al = 0;
    if (j.enhance) {
      r = blend8(0, r, fb); g = blend8(0, g, fb); b = blend8(0, b, fb);
      r = blend8(mean, r, fc); g = blend8(mean, g, fc); b = blend8(mean, b, fc);
      const int L = luma8(r, g, b);
      r = blend8(L, r, fs); g = blend8(L, g, fs); b = blend8(L, b, fs);
    }
    dst[i] = pack4(r, g, b, j.opacity[al]);
  }
}

// ---------------------------------------------------------------------------------------------- stage 8: paste, one thread per IMAGE pixel
// A pixel's thread applies the slots that cover it in slot order, so overlapping logos need no ordering between workgroups.
__global__ __launch_bounds__(256) void synth_paste_kernel(Args a, int K, uint8_t* __restrict__ images, size_t image_bytes, const ImageDesc* __restrict__ image_descs,
                                                          uint8_t* __restrict__ masks, size_t mask_bytes, const ImageDesc* __restrict__ mask_descs) {
  __shared__ const uint32_t* patch[kSynthMaxSlots];
  __shared__ int px[kSynthMaxSlots], py[kSynthMaxSlots], pw[kSynthMaxSlots], ph[kSynthMaxSlots];
  const int per = K * kB, n = blockIdx.x / per, blk = blockIdx.x % per;
  if ((int)threadIdx.x < K) {
    const int job = n * K + threadIdx.x;
    Plan p;
    pw[threadIdx.x] = 0;
    if (make_plan(a.jobs[job], a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p)) {
      patch[threadIdx.x] = stage_dst(p, slice_of(a.ws, job, a.P, a.T), S_FINISH);
      px[threadIdx.x] = a.jobs[job].x; py[threadIdx.x] = a.jobs[job].y; pw[threadIdx.x] = p.w[S_END]; ph[threadIdx.x] = p.h[S_END];
    }
  }
  __syncthreads();
  const ImageDesc d = image_descs[n];
  if (!rgb_desc_ok(d, image_bytes)) return;
  bool with_mask = masks != nullptr;
  ImageDesc md = d;
  if (with_mask) {
    md = mask_descs[n];
    with_mask = mask_desc_ok(md, d, mask_bytes);
  }
  uint8_t* __restrict__ img = images + d.offset;
  uint8_t* __restrict__ msk = with_mask ? masks + md.offset : nullptr;
  const int total = d.h * d.w;
  for (int i = blk * 256 + threadIdx.x; i < total; i += per * 256) {
    const int y = i / d.w, x = i - y * d.w;
    int r = 0, g = 0, b = 0, m = 0;
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
    if (msk) msk[i] = (uint8_t)m;
  }
}

// the finished patches, for the stage-level tests: job j's w x h RGBA patch -> out + j * P * 4
__global__ __launch_bounds__(256) void synth_export_kernel(Args a, uint32_t* __restrict__ out) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  Plan p;
  if (!make_plan(a.jobs[job], a.logo_descs, a.num_logos, a.logo_bytes, a.P, a.T, p)) return;
  const uint32_t* __restrict__ src = stage_dst(p, slice_of(a.ws, job, a.P, a.T), S_FINISH);
  const int total = p.w[S_END] * p.h[S_END];
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) out[(size_t)job * a.P + i] = src[i];
}

hipError_t launch_stages(const Args& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.J * kB)), block(256);
  hipLaunchKernelGGL(synth_tables_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(synth_resample_kernel, grid, block, 0, st, a, (int)S_R1H);
  hipLaunchKernelGGL(synth_resample_kernel, grid, block, 0, st, a, (int)S_R1V);
  hipLaunchKernelGGL(synth_rotate_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(synth_resample_kernel, grid, block, 0, st, a, (int)S_R3H);
  hipLaunchKernelGGL(synth_resample_kernel, grid, block, 0, st, a, (int)S_R3V);
  hipLaunchKernelGGL(synth_shear_kernel, grid, block, 0, st, a);
  for (int pass = 0; pass < 6; ++pass) hipLaunchKernelGGL(synth_blur_kernel, grid, block, 0, st, a, pass);
  hipLaunchKernelGGL(synth_luma_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(synth_finish_kernel, grid, block, 0, st, a);
  return hipGetLastError();
}

}  // namespace

size_t synth_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps) {
  if (N < 1 || K < 1 || K > kSynthMaxSlots || max_patch_pixels < 1 || max_patch_pixels > kSynthMaxPatchPixels || max_taps < 1 ||
      max_taps > kSynthMaxTaps || (long long)N * K > 2147483647ll / (kB * 4))
    return 0;
  return (size_t)N * K * ((size_t)8 * max_patch_pixels + (size_t)16 * max_taps + (size_t)8 * kB);
}

int synth_lanczos_ksize(int in, int out) {
  const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(3.0 * fs) * 2 + 1;
}

hipError_t launch_lanczos_table(int in, int out, int* table, hipStream_t st) {
  if (in < 1 || out < 1 || in > kMaxSide || out > kMaxSide || !table) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lanczos_table_kernel, dim3((unsigned)((out + 255) / 256)), dim3(256), 0, st, in, out, synth_lanczos_ksize(in, out), table);
  return hipGetLastError();
}

static bool synth_args_ok(const uint8_t* logos, size_t logo_bytes, const ImageDesc* logo_descs, int num_logos, const SynthJob* jobs, int N, int K,
                          long long P, long long T, void* ws, size_t ws_bytes) {
  const size_t need = synth_workspace_bytes(N, K, P, T);
  return logos && logo_descs && jobs && ws && logo_bytes >= 1 && num_logos >= 1 && need != 0 && ws_bytes >= need && !((uintptr_t)logos & 3) &&
         !(((uintptr_t)logo_descs | (uintptr_t)jobs | (uintptr_t)ws) & 7);
}

hipError_t launch_synth_u8(uint8_t* images, size_t image_bytes, const ImageDesc* image_descs, uint8_t* masks, size_t mask_bytes,
                           const ImageDesc* mask_descs, const uint8_t* logos, size_t logo_bytes, const ImageDesc* logo_descs, int num_logos,
                           const SynthJob* jobs, int N, int K, long long P, long long T, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!synth_args_ok(logos, logo_bytes, logo_descs, num_logos, jobs, N, K, P, T, ws, ws_bytes) || !images || !image_descs || image_bytes < 1 ||
      ((uintptr_t)image_descs & 7) || (masks && (!mask_descs || mask_bytes < 1 || ((uintptr_t)mask_descs & 7))))
    return hipErrorInvalidValue;
  const Args a{logos, logo_bytes, logo_descs, num_logos, jobs, N * K, (int)P, (int)T, ws};
  const hipError_t e = launch_stages(a, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(synth_paste_kernel, dim3((unsigned)(N * K * kB)), dim3(256), 0, st, a, K, images, image_bytes, image_descs, masks, mask_bytes,
                     mask_descs);
  return hipGetLastError();
}

hipError_t launch_synth_patches(const uint8_t* logos, size_t logo_bytes, const ImageDesc* logo_descs, int num_logos, const SynthJob* jobs, int J,
                                long long P, long long T, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, hipStream_t st) {
  if (!synth_args_ok(logos, logo_bytes, logo_descs, num_logos, jobs, J, 1, P, T, ws, ws_bytes) || !out || ((uintptr_t)out & 3) ||
      out_bytes / 4 / (size_t)P < (size_t)J)
    return hipErrorInvalidValue;
  const Args a{logos, logo_bytes, logo_descs, num_logos, jobs, J, (int)P, (int)T, ws};
  const hipError_t e = launch_stages(a, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(synth_export_kernel, dim3((unsigned)(J * kB)), dim3(256), 0, st, a, (uint32_t*)out);
  return hipGetLastError();
}

}  // namespace uwm
