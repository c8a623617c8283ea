// Everything a synthesis chain needs apart from its own stage list: the plan and its resize rule, the workspace slice, the choice of
// the ping-pong buffers, the kernels of the stages that the logo chain (synth_u8.hip) and the text chain (synth_text_u8.hip) have in
// common, and the host side.  Included after synth_stages.inc.  A chain is a recipe type C:
//   typedef ... Job;                          the ABI's job struct (SynthJob, TextJob)
//   enum { kTables, kStages, kRot, kBlur0, kFinish };      LANCZOS tables per job; S_END and the stages of rotate, blur pass 0, finish
//   static constexpr bool kReadsAtlas;        the first stage that runs reads the source atlas as RGBA (else a stage of the chain's own fills buffer 0)
//   static constexpr bool kSkipsBareImages;   paste leaves an image without a patch as it is, mask included
//   static int stage_of(int t);               the resample stage that LANCZOS table t serves: an even table a horizontal pass, t + 1 its vertical one
//   static bool make_plan(job, src_descs, num_src, src_bytes, P, T, plan);
//   static bool luma_factor(job, float& fb);  does finish need the Contrast mean, and the brightness factor in front of it
//   static int paste_mode(int mask_mode);     the mask rule of paste (kMask*)
//   static hipError_t launch_stages(args, stream);

template <int kStages, int kTables>
struct ChainPlan {
  long long off;                           // the source's byte offset in the atlas
  int w[kStages + 1], h[kStages + 1];      // size in front of stage s; [kStages] = the finished patch
  int before[kStages + 1];                 // stages that ran in front of stage s
  bool run[kStages];
  int ks[kTables];                         // taps per output of the LANCZOS tables
};
template <class C> using PlanOf = ChainPlan<C::kStages, C::kTables>;

// the table of a resample stage, -1 for any other stage
template <class C>
__device__ __forceinline__ int table_of(int s) {
  for (int t = 0; t < C::kTables; ++t) if (C::stage_of(t) == s) return t;
  return -1;
}

__device__ __forceinline__ bool side_ok(int v) { return v >= 1 && v <= kMaxSide; }
__device__ __forceinline__ bool patch_fits(int a, int b, int P) { return (long long)a * b <= (long long)P; }
__device__ __forceinline__ bool place_ok(int x, int y) { return x >= -(1 << 30) && x <= (1 << 30) && y >= -(1 << 30) && y <= (1 << 30); }

template <class C>
__device__ __forceinline__ void plan_clear(PlanOf<C>& p) {
  for (int s = 0; s < C::kStages; ++s) p.run[s] = false;
  for (int t = 0; t < C::kTables; ++t) p.ks[t] = 0;
}
// one Image.resize((tw, th), LANCZOS) of the w x h patch in front of stages sh (horizontal pass) and sh + 1 (vertical); an equal
// side has no pass.  `on` false: no resize, both stages are off
template <class C>
__device__ __forceinline__ bool plan_resize(PlanOf<C>& p, int& w, int& h, int sh, bool on, int tw, int th, int P, int T) {
  auto table_ok = [T](int in, int out, int& ks) { ks = lanczos_ksize(in, out); return (long long)out * (ks + 2) <= (long long)T; };
  if (!on) { p.w[sh] = p.w[sh + 1] = w; p.h[sh] = p.h[sh + 1] = h; return true; }
  if (!side_ok(tw) || !side_ok(th)) return false;
  p.w[sh] = w; p.h[sh] = h;
  if (tw != w) { p.run[sh] = true; if (!patch_fits(tw, h, P) || !table_ok(w, tw, p.ks[table_of<C>(sh)])) return false; w = tw; }
  p.w[sh + 1] = w; p.h[sh + 1] = h;
  if (th != h) { p.run[sh + 1] = true; if (!patch_fits(w, th, P) || !table_ok(h, th, p.ks[table_of<C>(sh + 1)])) return false; h = th; }
  return true;
}
// Pillow's rotate(expand) to w2 x h2 in front of stage C::kRot
template <class C>
__device__ __forceinline__ bool plan_rotate(PlanOf<C>& p, int& w, int& h, const typename C::Job& j, int P) {
  p.w[C::kRot] = w; p.h[C::kRot] = h;
  if (!j.rotate) return true;
  if (!side_ok(j.w2) || !side_ok(j.h2) || !patch_fits(j.w2, j.h2, P)) return false;
  for (int i = 0; i < 6; ++i) if (!finite_small(j.rot[i])) return false;
  p.run[C::kRot] = true; w = j.w2; h = j.h2;
  return true;
}
// the six box passes of GaussianBlur
template <class C>
__device__ __forceinline__ bool plan_blur(PlanOf<C>& p, const typename C::Job& j) {
  if (!j.blur) return true;
  if (j.blur_r < 0 || j.blur_r > kMaxBlurR) return false;
  for (int s = 0; s < 6; ++s) p.run[C::kBlur0 + s] = true;
  return true;
}
template <class C>
__device__ __forceinline__ void plan_count(PlanOf<C>& p) {
  int c = 0;
  for (int s = 0; s <= C::kStages; ++s) { p.before[s] = c; if (s < C::kStages && p.run[s]) ++c; }
}

// the workspace slice of one job: two patch buffers, the tables, the luma partial sums
template <int kTables> struct Slice { uint32_t* buf[2]; int* tab[kTables]; long long* part; };
template <int kTables>
__host__ __device__ __forceinline__ size_t slice_bytes(long long P, long long T) { return (size_t)8 * P + (size_t)4 * kTables * T + (size_t)8 * kSynthBlocks; }
template <int kTables>
__device__ __forceinline__ Slice<kTables> slice_of(void* ws, int job, int P, int T) {
  uint8_t* b = (uint8_t*)ws + (size_t)job * slice_bytes<kTables>(P, T);
  Slice<kTables> s;
  s.buf[0] = (uint32_t*)b; s.buf[1] = (uint32_t*)(b + (size_t)4 * P);
  for (int t = 0; t < kTables; ++t) s.tab[t] = (int*)(b + (size_t)8 * P + (size_t)4 * T * t);
  s.part = (long long*)(b + (size_t)8 * P + (size_t)4 * kTables * T);
  return s;
}

template <class C>
struct Args {
  const uint8_t* src; size_t src_bytes; const ImageDesc* src_descs; int num_src;       // the atlas: RGBA logos, coverage planes
  const typename C::Job* jobs; int J, P, T; void* ws;
};
template <class C>
__device__ __forceinline__ bool plan_of(const Args<C>& a, int job, PlanOf<C>& p) {
  return C::make_plan(a.jobs[job], a.src_descs, a.num_src, a.src_bytes, a.P, a.T, p);
}
template <class C>
__device__ __forceinline__ Slice<C::kTables> slice_of(const Args<C>& a, int job) { return slice_of<C::kTables>(a.ws, job, a.P, a.T); }

// the c-th stage that runs reads buffer (c - 1) & 1 and writes buffer c & 1; with kReadsAtlas the first one reads the atlas
template <class C>
__device__ __forceinline__ const uint32_t* stage_src(const Args<C>& a, const PlanOf<C>& p, const Slice<C::kTables>& sl, int s) {
  if (C::kReadsAtlas && p.before[s] == 0) return (const uint32_t*)(a.src + p.off);
  return sl.buf[(p.before[s] - 1) & 1];
}
template <class C>
__device__ __forceinline__ uint32_t* stage_dst(const PlanOf<C>& p, const Slice<C::kTables>& sl, int s) { return sl.buf[p.before[s] & 1]; }
// (the finish stage always runs, so something has been written)
template <class C>
__device__ __forceinline__ const uint32_t* finished(const PlanOf<C>& p, const Slice<C::kTables>& sl) { return sl.buf[(p.before[C::kStages] - 1) & 1]; }

// ---------------------------------------------------------------------------------------------- the stages both chains have
template <class C>
__global__ __launch_bounds__(256) void chain_tables_kernel(Args<C> a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  PlanOf<C> p;
  if (!plan_of(a, job, p)) return;
  const Slice<C::kTables> sl = slice_of(a, job);
  for (int t = 0; t < C::kTables; ++t) {
    const int s = C::stage_of(t);
    if (!p.run[s]) continue;
    const bool horiz = !(t & 1);
    lanczos_rows(horiz ? p.w[s] : p.h[s], horiz ? p.w[s + 1] : p.h[s + 1], p.ks[t], sl.tab[t], blk);
  }
}

// one pass of a resize: stage s is a horizontal pass when its table is even, and s + 1 is then the vertical pass of the same resize
template <class C>
__global__ __launch_bounds__(256) void chain_resample_kernel(Args<C> a, int s) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  PlanOf<C> p;
  if (!plan_of(a, job, p) || !p.run[s]) return;
  const Slice<C::kTables> sl = slice_of(a, job);
  const int t = table_of<C>(s);
  const bool horiz = !(t & 1);
  const bool premul = horiz || !p.run[s - 1];          // the first pass of this resize that runs
  const bool unpremul = !horiz || !p.run[s + 1];       // the last one
  resample_pass(stage_src(a, p, sl, s), stage_dst<C>(p, sl, s), p.w[s], p.w[s + 1], p.h[s + 1], sl.tab[t], p.ks[t], horiz, premul, unpremul, blk);
}

template <class C>
__global__ __launch_bounds__(256) void chain_rotate_kernel(Args<C> a) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  PlanOf<C> p;
  if (!plan_of(a, job, p) || !p.run[C::kRot]) return;
  const Slice<C::kTables> sl = slice_of(a, job);
  rotate_pass(stage_src(a, p, sl, C::kRot), stage_dst<C>(p, sl, C::kRot), p.w[C::kRot], p.h[C::kRot], p.w[C::kRot + 1], p.h[C::kRot + 1],
              a.jobs[job].rot, blk);
}

template <class C>
__global__ __launch_bounds__(256) void chain_blur_kernel(Args<C> a, int pass) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  const typename C::Job& j = a.jobs[job];
  const int s = C::kBlur0 + pass;
  PlanOf<C> p;
  if (!plan_of(a, job, p) || !p.run[s]) return;
  const Slice<C::kTables> sl = slice_of(a, job);
  blur_pass(stage_src(a, p, sl, s), stage_dst<C>(p, sl, s), p.w[s], p.h[s], j.blur_r, j.blur_ww, j.blur_fw, pass < 3, blk);
}

// per-workgroup partial sums of L over the brightened patch (the Contrast degenerate is their mean); integer sums: any order, one result
template <class C>
__global__ __launch_bounds__(256) void chain_luma_kernel(Args<C> a) {
  __shared__ long long red[256];
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  PlanOf<C> p;
  float fb;
  if (!plan_of(a, job, p) || !C::luma_factor(a.jobs[job], fb)) return;      // uniform over the workgroup
  const Slice<C::kTables> sl = slice_of(a, job);
  luma_partial(stage_src(a, p, sl, C::kFinish), p.w[C::kFinish] * p.h[C::kFinish], fb, blk, red, sl.part + blk);
}

// the finished patches, for the stage-level tests: job j's w x h RGBA patch -> out + j * P * 4
template <class C>
__global__ __launch_bounds__(256) void chain_export_kernel(Args<C> a, uint32_t* __restrict__ out) {
  const int job = blockIdx.x / kB, blk = blockIdx.x % kB;
  PlanOf<C> p;
  if (!plan_of(a, job, p)) return;
  const uint32_t* __restrict__ src = finished<C>(p, slice_of(a, job));
  const int total = p.w[C::kStages] * p.h[C::kStages];
  for (int i = blk * 256 + threadIdx.x; i < total; i += kB * 256) out[(size_t)job * a.P + i] = src[i];
}

// Paste, one thread per IMAGE pixel.  A pixel's thread applies the slots that cover it in slot order, so overlapping patches need no
// ordering between workgroups, and it forms its own mask byte, so a halving happens once whatever K is.  The mask rule:
enum {
  kMaskOver = 0,       // paste over what the plane holds; a pixel no patch covers keeps its byte
  kMaskHalve = 1,      // paste from 0, then max(byte >> 1, that)
  kMaskWrite = 2       // paste from 0 and write every pixel
};
template <class C>
__global__ __launch_bounds__(256) void chain_paste_kernel(Args<C> a, int K, uint8_t* __restrict__ images, size_t image_bytes, const ImageDesc* __restrict__ image_descs,
                                                          uint8_t* __restrict__ masks, size_t mask_bytes, const ImageDesc* __restrict__ mask_descs, int mask_mode) {
  __shared__ const uint32_t* patch[kSynthMaxSlots];
  __shared__ int px[kSynthMaxSlots], py[kSynthMaxSlots], pw[kSynthMaxSlots], ph[kSynthMaxSlots];
  const int per = K * kB, n = blockIdx.x / per, blk = blockIdx.x % per;
  const int mode = C::paste_mode(mask_mode);
  if ((int)threadIdx.x < K) {
    const int job = n * K + threadIdx.x;
    PlanOf<C> p;
    pw[threadIdx.x] = 0;
    if (plan_of(a, job, p)) {
      patch[threadIdx.x] = finished<C>(p, slice_of(a, job));
      px[threadIdx.x] = a.jobs[job].x; py[threadIdx.x] = a.jobs[job].y; pw[threadIdx.x] = p.w[C::kStages]; ph[threadIdx.x] = p.h[C::kStages];
    }
  }
  __syncthreads();
  if (C::kSkipsBareImages) {
    bool any = false;
    for (int k = 0; k < K; ++k) any |= pw[k] != 0;
    if (!any) return;
  }
  const ImageDesc d = image_descs[n];
  if (!region_ok(d, 3, image_bytes, 1, kMaxSide)) return;
  uint8_t* __restrict__ img = images + d.offset;
  uint8_t* __restrict__ msk = nullptr;
  if (masks) {
    const ImageDesc md = mask_descs[n];
    if (md.h == d.h && md.w == d.w && region_ok(md, 1, mask_bytes, 1, kMaxSide)) msk = masks + md.offset;
  }
  const int total = d.h * d.w;
  for (int i = blk * 256 + threadIdx.x; i < total; i += per * 256) {
    const int y = i / d.w, x = i - y * d.w;
    int r = 0, g = 0, b = 0;
    int m = (msk && mode == kMaskOver) ? msk[i] : 0;
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
      if (mode == kMaskHalve) msk[i] = (uint8_t)max((int)msk[i] >> 1, m);
      else if (mode == kMaskWrite || loaded) msk[i] = (uint8_t)m;
    }
  }
}

// ---------------------------------------------------------------------------------------------- host side
template <class C>
size_t chain_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps) {
  if (N < 1 || K < 1 || K > kSynthMaxSlots || max_patch_pixels < 1 || max_patch_pixels > kSynthMaxPatchPixels || max_taps < 1 ||
      max_taps > kSynthMaxTaps || (long long)N * K > 2147483647ll / (kB * 4))
    return 0;
  return (size_t)N * K * slice_bytes<C::kTables>(max_patch_pixels, max_taps);
}

template <class C>
bool chain_args_ok(const uint8_t* src, size_t src_bytes, const ImageDesc* src_descs, int num_src, const typename C::Job* jobs, int N, int K, long long P,
                   long long T, void* ws, size_t ws_bytes) {
  const size_t need = chain_workspace_bytes<C>(N, K, P, T);
  return src && src_descs && jobs && ws && src_bytes >= 1 && num_src >= 1 && need != 0 && ws_bytes >= need && !((uintptr_t)src & 3) &&
         !(((uintptr_t)src_descs | (uintptr_t)jobs | (uintptr_t)ws) & 7);
}

// the stages of N * K jobs, then the paste into the N images
template <class C>
hipError_t launch_chain_batch(uint8_t* images, size_t image_bytes, const ImageDesc* image_descs, uint8_t* masks, size_t mask_bytes,
                              const ImageDesc* mask_descs, int mask_mode, const uint8_t* src, size_t src_bytes, const ImageDesc* src_descs,
                              int num_src, const typename C::Job* jobs, int N, int K, long long P, long long T, void* ws, size_t ws_bytes,
                              hipStream_t st) {
  if (!chain_args_ok<C>(src, src_bytes, src_descs, num_src, jobs, N, K, P, T, ws, ws_bytes) || !images || !image_descs || image_bytes < 1 ||
      ((uintptr_t)image_descs & 7) || (masks && (!mask_descs || mask_bytes < 1 || ((uintptr_t)mask_descs & 7))))
    return hipErrorInvalidValue;
  const Args<C> a{src, src_bytes, src_descs, num_src, jobs, N * K, (int)P, (int)T, ws};
  UWM_CHK(C::launch_stages(a, st));
  hipLaunchKernelGGL(chain_paste_kernel<C>, dim3((unsigned)(N * K * kB)), dim3(256), 0, st, a, K, images, image_bytes, image_descs, masks, mask_bytes,
                     mask_descs, mask_mode);
  return hipGetLastError();
}

// the stages of J jobs, then their finished patches -> out
template <class C>
hipError_t launch_chain_patches(const uint8_t* src, size_t src_bytes, const ImageDesc* src_descs, int num_src, const typename C::Job* jobs, int J,
                                long long P, long long T, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, hipStream_t st) {
  if (!chain_args_ok<C>(src, src_bytes, src_descs, num_src, jobs, J, 1, P, T, ws, ws_bytes) || !out || ((uintptr_t)out & 3) ||
      out_bytes / 4 / (size_t)P < (size_t)J)
    return hipErrorInvalidValue;
  const Args<C> a{src, src_bytes, src_descs, num_src, jobs, J, (int)P, (int)T, ws};
  UWM_CHK(C::launch_stages(a, st));
  hipLaunchKernelGGL(chain_export_kernel<C>, dim3((unsigned)(J * kB)), dim3(256), 0, st, a, (uint32_t*)out);
  return hipGetLastError();
}
