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

#include "image_common.inc"
#include "synth_stages.inc"
#include "synth_chain.inc"

enum { S_R1H = 0, S_R1V, S_ROT, S_R3H, S_R3V, S_SHEAR, S_BLUR0, S_FINISH = S_BLUR0 + 6, S_END };

// the logo chain's recipe (synth_chain.inc)
struct Logo {
  typedef SynthJob Job;
  enum { kTables = 4, kStages = S_END, kRot = S_ROT, kBlur0 = S_BLUR0, kFinish = S_FINISH };      // tables: r1h, r1v, r3h, r3v
  typedef ChainPlan<kStages, kTables> Plan;
  static constexpr bool kReadsAtlas = true, kSkipsBareImages = false;
  static __device__ __forceinline__ int stage_of(int t) { return t == 0 ? S_R1H : t == 1 ? S_R1V : t == 2 ? S_R3H : S_R3V; }
  static __device__ __forceinline__ bool luma_factor(const Job& j, float& fb) { fb = j.brightness; return j.enhance != 0; }
  static __device__ __forceinline__ int paste_mode(int) { return kMaskWrite; }
  static __device__ bool make_plan(const SynthJob& j, const ImageDesc* __restrict__ logo_descs, int num_logos, size_t logo_bytes, int P, int T, Plan& p);
  static hipError_t launch_stages(const Args<Logo>& a, hipStream_t st);
};

// the one place that decides whether job j runs: true only if every read and write of every stage stays inside its buffer
__device__ bool Logo::make_plan(const SynthJob& j, const ImageDesc* __restrict__ logo_descs, int num_logos, size_t logo_bytes, int P, int T, Plan& p) {
  if (!j.enabled || j.logo < 0 || j.logo >= num_logos) return false;
  const ImageDesc ld = logo_descs[j.logo];
  if ((ld.offset & 3) || !region_ok(ld, 4, logo_bytes, 1, kMaxSide)) return false;
  p.off = ld.offset;
  int w = ld.w, h = ld.h;
  plan_clear<Logo>(p);
  if (!plan_resize<Logo>(p, w, h, S_R1H, true, j.w1, j.h1, P, T)) return false;
  if (!plan_rotate<Logo>(p, w, h, j, P)) return false;
  if (!plan_resize<Logo>(p, w, h, S_R3H, j.stretch != 0, j.w3, j.h3, P, T)) return false;
  p.w[S_SHEAR] = w; p.h[S_SHEAR] = h;
  if (j.stretch && j.shear) {
    for (int i = 0; i < 6; ++i) if (!finite_small(j.shear_minv[i])) return false;
    p.run[S_SHEAR] = true;
  }
  if (!plan_blur<Logo>(p, j)) return false;
  for (int s = S_BLUR0; s <= S_END; ++s) { p.w[s] = w; p.h[s] = h; }
  if (!patch_fits(w, h, P)) return false;              // (no stage ran: the logo itself must fit the buffer finish writes)
  if (j.ndefects < 0 || j.ndefects > 3) return false;
  for (int d = 0; d < j.ndefects; ++d)
    for (int i = 0; i < 4; ++i) if (j.defects[d][i] < 0 || j.defects[d][i] > kMaxSide) return false;
  if (!place_ok(j.x, j.y)) return false;
  p.run[S_FINISH] = true;
  plan_count<Logo>(p);
  return true;
}

// ---------------------------------------------------------------------------------------------- LANCZOS tables
__global__ __launch_bounds__(256) void lanczos_table_kernel(int in, int out, int ksize, int* __restrict__ table) {
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx < out) lanczos_row(in, out, ksize, xx, table + (size_t)xx * (ksize + 2));
}

// ---------------------------------------------------------------------------------------------- stage 3b: shear (restated; NOT run against cv2)
__device__ __forceinline__ long long rne1024(double v) { return (long long)rint(__dmul_rn(v, 1024.0)); }

__global__ __launch_bounds__(256) void synth_shear_kernel(Args<Logo> a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const SynthJob& j = a.jobs[job];
  Logo::Plan p;
  if (!plan_of(a, job, p) || !p.run[S_SHEAR]) return;
  const auto sl = slice_of(a, job);
  const uint32_t* __restrict__ src = stage_src(a, p, sl, S_SHEAR);
  uint32_t* __restrict__ dst = stage_dst<Logo>(p, sl, S_SHEAR);
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

// ---------------------------------------------------------------------------------------------- stages 5-7: defects, the three enhancers, opacity
__global__ __launch_bounds__(256) void synth_finish_kernel(Args<Logo> a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const SynthJob& j = a.jobs[job];
  Logo::Plan p;
  if (!plan_of(a, job, p)) return;
  const auto sl = slice_of(a, job);
  const uint32_t* __restrict__ src = stage_src(a, p, sl, S_FINISH);
  uint32_t* __restrict__ dst = stage_dst<Logo>(p, sl, S_FINISH);
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

// 15 launches: tables, 2 passes of the first resize, rotate, 2 passes of the stretch, shear, 6 blur passes, the Contrast mean, finish
hipError_t Logo::launch_stages(const Args<Logo>& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.J * kB)), block(256);
  hipLaunchKernelGGL(chain_tables_kernel<Logo>, grid, block, 0, st, a);
  hipLaunchKernelGGL(chain_resample_kernel<Logo>, grid, block, 0, st, a, (int)S_R1H);
  hipLaunchKernelGGL(chain_resample_kernel<Logo>, grid, block, 0, st, a, (int)S_R1V);
  hipLaunchKernelGGL(chain_rotate_kernel<Logo>, grid, block, 0, st, a);
  hipLaunchKernelGGL(chain_resample_kernel<Logo>, grid, block, 0, st, a, (int)S_R3H);
  hipLaunchKernelGGL(chain_resample_kernel<Logo>, grid, block, 0, st, a, (int)S_R3V);
  hipLaunchKernelGGL(synth_shear_kernel, grid, block, 0, st, a);
  for (int pass = 0; pass < 6; ++pass) hipLaunchKernelGGL(chain_blur_kernel<Logo>, grid, block, 0, st, a, pass);
  hipLaunchKernelGGL(chain_luma_kernel<Logo>, grid, block, 0, st, a);
  hipLaunchKernelGGL(synth_finish_kernel, grid, block, 0, st, a);
  return hipGetLastError();
}

}  // namespace

size_t synth_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps) {
  return chain_workspace_bytes<Logo>(N, K, max_patch_pixels, max_taps);
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

hipError_t launch_synth_u8(uint8_t* images, size_t image_bytes, const ImageDesc* image_descs, uint8_t* masks, size_t mask_bytes,
                           const ImageDesc* mask_descs, const uint8_t* logos, size_t logo_bytes, const ImageDesc* logo_descs, int num_logos,
                           const SynthJob* jobs, int N, int K, long long P, long long T, void* ws, size_t ws_bytes, hipStream_t st) {
  return launch_chain_batch<Logo>(images, image_bytes, image_descs, masks, mask_bytes, mask_descs, 0, logos, logo_bytes, logo_descs, num_logos, jobs,
                                  N, K, P, T, ws, ws_bytes, st);
}

hipError_t launch_synth_patches(const uint8_t* logos, size_t logo_bytes, const ImageDesc* logo_descs, int num_logos, const SynthJob* jobs, int J,
                                long long P, long long T, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, hipStream_t st) {
  return launch_chain_patches<Logo>(logos, logo_bytes, logo_descs, num_logos, jobs, J, P, T, ws, ws_bytes, out, out_bytes, st);
}

}  // namespace uwm
