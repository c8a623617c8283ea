// libuwm, part of uwm_model.hip (one translation unit; included from there): the C ABI of include/uwm.h (extern "C" entry points, single-operator entry points for tests and kernel timing).
// ------------------------------------------------------------------------------ C ABI
extern "C" {

const char* uwm_last_error(void) { return g_err; }
int uwm_version(void) { return 1; }

int uwm_create(const uwm_unet_desc* desc, uwm_handle* out) {
  if (!desc || !out) return fail("uwm_create: null argument");
  uwm_model* m = new uwm_model();
  m->desc = *desc;
  if (m->desc.bn_eps <= 0.f) m->desc.bn_eps = 1e-5f;
  if (m->desc.bn_momentum <= 0.f) m->desc.bn_momentum = 0.1f;
  if (build_model(m)) { delete m; return 1; }
  const char* e = getenv("UWM_SIDE_STREAM");
  m->use_side = e ? atoi(e) : 1;
  if (const char* pe = getenv("UWM_PRECISION")) {      // process default of the precision mode (like UWM_WINOGRAD): f32 | bf16x3 | bf16x3_all | f16x3 | f16x3_all or 0..4
    static const char* names[7] = {"f32", "bf16x3", "bf16x3_all", "f16x3", "f16x3_all", "f16x1", "f16x3_bwd2"};
    int found = -1;
    for (int i = 0; i < 7; ++i) if (!strcmp(pe, names[i]) || (pe[0] == '0' + i && !pe[1])) found = i;
    if (found < 0) { delete m; return fail("uwm_create: UWM_PRECISION=%s is not a precision mode (f32 | bf16x3 | bf16x3_all | f16x3 | f16x3_all | f16x1 | f16x3_bwd2 or 0..6)", pe); }
    m->prec = found; m->plan.prec = found; m->prec_from_env = found != UWM_PREC_F32;
  }
  if (const char* pf = getenv("UWM_F16X3_MIN_WGS")) m->f3_min_wgs = atoi(pf) > 0 ? atoi(pf) : 0;      // process default of uwm_set_precision_fill
  m->wino_mode = winograd_mode();       // process default (UWM_WINOGRAD / uwm_set_winograd) at creation; then per handle
  m->plan.wino_mode = m->wino_mode;
  *out = m; return 0;
}
void uwm_destroy(uwm_handle h) {
  if (!h) return;
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_pack) (void)hipEventDestroy(h->ev_pack);
  if (h->ev_disp) (void)hipEventDestroy(h->ev_disp);
  if (h->side) (void)hipStreamDestroy(h->side);
  delete h;
}

long long uwm_param_arena_floats(uwm_handle h) { return h ? h->param_floats : 0; }
long long uwm_buffer_arena_floats(uwm_handle h) { return h ? h->buffer_floats : 0; }
long long uwm_param_count(uwm_handle h) { return h ? h->param_count : 0; }
int uwm_num_tensors(uwm_handle h) { return h ? (int)h->infos.size() : 0; }
int uwm_tensor_info_get(uwm_handle h, int i, uwm_tensor_info* out) {
  if (!h || !out || i < 0 || i >= (int)h->infos.size()) return fail("uwm_tensor_info_get: bad index %d", i);
  *out = h->infos[i]; return 0;
}
int uwm_logits_channels(uwm_handle h) { return h ? h->CP : 0; }
int uwm_num_stages(uwm_handle h) { return h ? h->nstages : 0; }
int uwm_stage_range(uwm_handle h, int stage, long long* b, long long* e) {
  if (!h || stage < 0 || stage >= h->nstages || !b || !e) return fail("uwm_stage_range: bad stage %d", stage);
  *b = h->stage_begin[stage]; *e = h->stage_begin[stage + 1]; return 0;
}
// RAII: make `dev` the current HIP device for the scope of one ABI call (a handle is bound to the device its arenas
// live on; the caller's current device may be another one)
struct DeviceGuard {
  int prev = -1; bool switched = false;
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); return; }
    if (prev != dev && hipSetDevice(dev) == hipSuccess) switched = true;
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

int uwm_bind(uwm_handle h, float* params, float* grads, float* buffers) {
  if (!h || !params || !buffers) return fail("uwm_bind: params and buffers must be non-null");
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)buffers) & 15) return fail("uwm_bind: arenas must be 16-byte aligned");
  hipPointerAttribute_t at;
  int dev = -1;
  if (hipPointerGetAttributes(&at, params) == hipSuccess) dev = at.device; else (void)hipGetLastError();
  if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) { dev = -1; (void)hipGetLastError(); } }
  if (h->device >= 0 && h->device != dev && h->side) {      // arenas moved to another device: the side stream moves with them
    DeviceGuard g0(h->device);
    (void)hipStreamSynchronize(h->side);
    (void)hipEventDestroy(h->ev_fork); (void)hipEventDestroy(h->ev_join); (void)hipEventDestroy(h->ev_pack);
    if (h->ev_disp) (void)hipEventDestroy(h->ev_disp);
    (void)hipStreamDestroy(h->side);
    h->side = nullptr; h->ev_fork = h->ev_join = h->ev_pack = h->ev_disp = nullptr; h->packed_in_fwd = false;
  }
  h->device = dev;
  h->params = params; h->grads = grads; h->buffers = buffers;
  h->frozen = nullptr;                  // other arenas: whatever was frozen no longer describes them
  DeviceGuard guard(dev);
  if (h->use_side && !h->side) {        // created on the device the arenas live on
    // LOWEST queue priority: the weight gradients are off the critical path, the dgrad / BatchNorm-backward chain on the caller's
    // stream is it — when a CU slot frees up, the dependent chain's workgroups must get it first
    int prio_lo = 0, prio_hi = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) { prio_lo = 0; (void)hipGetLastError(); }
    if (dbg_flag("UWM_SIDE_PRIO_NORMAL")) prio_lo = 0;
    if (hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, prio_lo) != hipSuccess) { h->side = nullptr; (void)hipGetLastError(); }
    else if (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_pack, hipEventDisableTiming) != hipSuccess) {
      (void)hipStreamDestroy(h->side); h->side = nullptr; (void)hipGetLastError();
    }
    if (h->side && hipEventCreate(&h->ev_disp) != hipSuccess) { h->ev_disp = nullptr; (void)hipGetLastError(); }
    h->disp_fork = dbg_flag("UWM_NO_DISPATCH_FORK") ? 0 : 1;
    // ROCm maps HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) in creation order.  In a process that
    // has already created several streams (RCCL, torch) the side stream can alias the compute stream's queue: the
    // weight-gradient overlap is then silently lost (measured -5 %, DESIGN.md 6).  The variable is read when the HIP
    // runtime initialises, so all the library can do at this point is say so.
    if (h->side && !h->hwq_warned) {
      const char* q = getenv("GPU_MAX_HW_QUEUES");
      if (!q || atoi(q) < 8) {
        fprintf(stderr, "libuwm: warning: GPU_MAX_HW_QUEUES=%s (< 8): the weight-gradient side stream may share a hardware queue with "
                        "the compute stream and lose its overlap; export GPU_MAX_HW_QUEUES=8 before the HIP runtime starts\n", q ? q : "unset");
        h->hwq_warned = true;
      }
    }
  }
  return 0;
}

static int check_shape(int N, int H, int W) {
  if (N < 1) return fail("batch size must be >= 1, got %d", N);
  if (H < 32 || W < 32 || (H % 32) || (W % 32))
    return fail("Wrong input shape height=%d, width=%d. Expected image height and width divisible by 32.", H, W);
  if ((long long)N * H * W >= (1LL << 31) / 16) return fail("N*H*W too large for 32-bit pixel indexing: %lld", (long long)N * H * W);
  return 0;
}

size_t uwm_workspace_bytes(uwm_handle h, int N, int H, int W, int training) {
  if (!h || check_shape(N, H, W)) return 0;
  if (h->plan.N != N || h->plan.H != H || h->plan.W != W || h->plan.training != (training ? 1 : 0)) {
    make_plan(h, N, H, W, training ? 1 : 0);
    h->have_fwd = false;
  }
  return h->plan.bytes;
}

// Algorithmic (direct-convolution) FLOPs per IMAGE of this model at H x W — SURVEY.md 8(d)'s roofline numerator:
// forward = sum over conv layers of 2*Ho*Wo*Cout*Cin_per_group*k*k ; forward+backward = 3x that minus the stem's dgrad
// (the input image needs no gradient).  BatchNorm / elementwise / loss / optimizer work is not counted.
int uwm_conv_flops(uwm_handle h, int H, int W, double* fwd, double* fwd_bwd) {
  if (!h || !fwd || !fwd_bwd) return fail("uwm_conv_flops: null argument");
  if (check_shape(1, H, W)) return 1;
  const Plan keep = h->plan;
  make_plan(h, 1, H, W, 0);
  double f = 0.0, fb = 0.0;
  for (size_t ci = 0; ci < h->convs.size(); ++ci) {
    const ConvL& cv = h->convs[ci];
    const double macs = (double)h->plan.oh[ci] * h->plan.ow[ci] * cv.Cout * (cv.dw ? 1 : cv.Cin) * cv.k * cv.k;
    f += 2.0 * macs; fb += 2.0 * macs * ((int)ci == h->stem ? 2.0 : 3.0);
  }
  h->plan = keep;
  *fwd = f; *fwd_bwd = fb; return 0;
}

int uwm_forward(uwm_handle h, const float* x, float* logits, void* ws, size_t ws_bytes, int N, int H, int W, int training,
                uwm_stream stream) {
  if (!h || !x || !logits || !ws) return fail("uwm_forward: null argument");
  if (!h->params || !h->buffers) return fail("uwm_forward: call uwm_bind first");
  if (check_shape(N, H, W)) return 1;
  if (((uintptr_t)x | (uintptr_t)logits | (uintptr_t)ws) & 15) return fail("uwm_forward: pointers must be 16-byte aligned");
  const size_t need = uwm_workspace_bytes(h, N, H, W, training);
  if (ws_bytes < need) return fail("uwm_forward: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  h->have_fwd = false;
  DeviceGuard guard(h->device);
  if (do_forward(h, x, logits, (float*)ws, N, H, W, training ? 1 : 0, (hipStream_t)stream)) return 1;
  h->have_fwd = training != 0;
  return 0;
}

// ---- frozen-weight inference: the parameter-derived items of the eval forward, made once into a caller-owned arena
size_t uwm_frozen_bytes(uwm_handle h) { return h ? h->frozen_floats * sizeof(float) : 0; }
int uwm_is_frozen(uwm_handle h) { return h && h->frozen ? 1 : 0; }
int uwm_unfreeze(uwm_handle h) {
  if (!h) return fail("uwm_unfreeze: null handle");
  h->frozen = nullptr; return 0;
}
long long uwm_prep_launches(uwm_handle h) { return h ? h->prep_launches : 0; }
// the plan of an eval forward of (N, H, W) for the time of one call that only needs its routing (the held plan — a training forward
// waiting for its backward, say — comes back afterwards)
struct PlanScope {
  uwm_model* m; Plan keep; bool have_fwd;
  PlanScope(uwm_model* m_, int N, int H, int W) : m(m_), keep(m_->plan), have_fwd(m_->have_fwd) { make_plan(m, N, H, W, 0); }
  ~PlanScope() { m->plan = keep; m->have_fwd = have_fwd; }
};
int uwm_freeze(uwm_handle h, void* frozen, size_t bytes, int N, int H, int W, uwm_stream stream) {
  if (!h || !frozen) return fail("uwm_freeze: null argument");
  if (check_shape(N, H, W)) return 1;
  if ((uintptr_t)frozen & 15) return fail("uwm_freeze: the arena must be 16-byte aligned");
  if (bytes < uwm_frozen_bytes(h)) return fail("uwm_freeze: arena too small (%zu < %zu bytes)", bytes, uwm_frozen_bytes(h));
  if (!h->params || !h->buffers) return fail("uwm_freeze: call uwm_bind first");
  if (h->param_floats >= (1LL << 32) || h->buffer_floats >= (1LL << 32) || h->frozen_floats >= ((size_t)1 << 32))
    return fail("uwm_freeze: arena offsets do not fit the 32 bits of a BnEvalJob");
  h->frozen = nullptr;
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  PlanScope scope(h, N, H, W);
  Ctx c{h, nullptr, st, N};
  c.fz = (float*)frozen;
  BnEvalJobs jobs; jobs.n = 0;
  auto flush = [&]() -> hipError_t { if (jobs.n == 0) return hipSuccess; ++h->prep_launches; hipError_t e = launch_bn_eval_multi(h->params, h->buffers, c.fz, jobs, st); jobs.n = 0; return e; };
  for (auto& b : h->bns) {
    BnEvalJob& j = jobs.j[jobs.n++];
    j.g_off = (unsigned)b.g_off; j.rm_off = (unsigned)b.rm_off; j.out_off = (unsigned)b.fz_off; j.C = b.C;
    j.eps = b.eps > 0.f ? b.eps : h->desc.bn_eps;
    if (b.b_off != b.g_off + b.C || b.rv_off != b.rm_off + b.C) return fail("internal: uwm_freeze expects beta behind gamma and the running variance behind the mean");
    if (jobs.n == BnEvalJobs::kMax) LCHK(flush());
  }
  LCHK(flush());
  LCHK(wino_jobs(c, false, st));
  if (stem_bank_job(c, st)) return 1;
  h->fz_form.assign(h->convs.size(), 0);
  for (size_t ci = 0; ci < h->convs.size(); ++ci) h->fz_form[ci] = (signed char)fwd_bank_form(h, ci);
  h->frozen = (float*)frozen;
  return 0;
}
int uwm_frozen_serves(uwm_handle h, int N, int H, int W) {
  if (!h || !h->frozen || check_shape(N, H, W)) return 0;
  PlanScope scope(h, N, H, W);
  return frozen_serves(h) ? 1 : 0;
}
size_t uwm_predict_workspace_bytes(uwm_handle h, int N, int H, int W, int with_logits) {
  const size_t need = uwm_workspace_bytes(h, N, H, W, 0);
  return need && with_logits ? need + (size_t)N * H * W * h->CP * sizeof(float) : need;
}
int uwm_predict_u8(uwm_handle h, const uint8_t* images, const float* mean, const float* std, float threshold, int apply_sigmoid,
                   int out_h, int out_w, uint8_t* mask, float* logits, void* ws, size_t ws_bytes, int N, int H, int W,
                   uwm_stream stream) {
  if (!h || !images || !mean || !std || !mask || !ws) return fail("uwm_predict_u8: null argument");
  if (!h->params || !h->buffers) return fail("uwm_predict_u8: call uwm_bind first");
  if (check_shape(N, H, W)) return 1;
  if (out_h < 1 || out_w < 1) return fail("uwm_predict_u8: bad output size %d x %d", out_h, out_w);
  const int C = h->desc.in_channels;
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_predict_u8: std[%d] must be positive", c);
  if ((uintptr_t)images & 3) return fail("uwm_predict_u8: images must be 4-byte aligned");
  if (((uintptr_t)logits | (uintptr_t)ws) & 15) return fail("uwm_predict_u8: logits and workspace must be 16-byte aligned");
  const size_t need = uwm_predict_workspace_bytes(h, N, H, W, logits ? 0 : 1);
  if (ws_bytes < need) return fail("uwm_predict_u8: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  float* lg = logits ? logits : (float*)ws + h->plan.bytes / sizeof(float);      // (no caller buffer: behind the plan)
  h->have_fwd = false;
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  LCHK(launch_preprocess_u8_nhwc4(images, (size_t)N * H * W, C, mean, std, (float*)ws + h->plan.x4, st));
  if (do_forward(h, nullptr, lg, (float*)ws, N, H, W, 0, st)) return 1;
  LCHK(launch_resize_threshold(lg, h->CP, N, H, W, out_h, out_w, threshold, apply_sigmoid, mask, nullptr, st));
  return 0;
}
// ---- cv2-convention resize of ragged uint8 batches (resize_u8.hip): every argument is checked here, before any launch (the
// descriptors are device memory: the kernels clamp them)
static_assert(sizeof(uwm_image_desc) == sizeof(ImageDesc) && sizeof(uwm_image_desc) == 16, "uwm_image_desc layout");
static int resize_args_check(const char* fn, const void* src, size_t src_bytes, const void* descs, int N, int C, int H, int W, const void* out) {
  if (!src || !descs || !out) return fail("%s: null argument", fn);
  if (C < 1 || C > 4) return fail("%s: C must be 1..4 (got %d)", fn, C);
  if (N < 1 || H < 1 || W < 1 || src_bytes < 1) return fail("%s: N, H, W and src_bytes must be >= 1 (got %d, %d, %d, %zu)", fn, N, H, W, src_bytes);
  if ((long long)N * ((H + kResizeRowsPerBlock - 1) / kResizeRowsPerBlock) > 2147483647ll) return fail("%s: N * H too large for one launch (%d x %d)", fn, N, H);
  if ((uintptr_t)src & 3) return fail("%s: src must be 4-byte aligned", fn);
  if ((uintptr_t)descs & 7) return fail("%s: descriptors must be 8-byte aligned", fn);
  return 0;
}
int uwm_resize_u8(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int N, int C, int H, int W, int interp,
                  uint8_t* out, uwm_stream stream) {
  if (resize_args_check("uwm_resize_u8", src, src_bytes, descs, N, C, H, W, out)) return 1;
  if (interp != UWM_INTER_NEAREST && interp != UWM_INTER_LINEAR)
    return fail("uwm_resize_u8: unknown interp %d (UWM_INTER_NEAREST = 0 | UWM_INTER_LINEAR = 1)", interp);
  LCHK(launch_resize_u8(src, src_bytes, (const ImageDesc*)descs, N, C, H, W, interp, out, (hipStream_t)stream));
  return 0;
}
int uwm_op_resize_norm_u8_nhwc4(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int N, int C, int H, int W,
                                const float* mean, const float* std, float* out, uwm_stream stream) {
  if (resize_args_check("uwm_op_resize_norm_u8_nhwc4", src, src_bytes, descs, N, C, H, W, out)) return 1;
  if (!mean || !std) return fail("uwm_op_resize_norm_u8_nhwc4: null argument");
  if ((uintptr_t)out & 15) return fail("uwm_op_resize_norm_u8_nhwc4: out must be 16-byte aligned");
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_op_resize_norm_u8_nhwc4: std[%d] must be positive", c);
  LCHK(launch_resize_norm_u8_nhwc4(src, src_bytes, (const ImageDesc*)descs, N, C, H, W, mean, std, out, (hipStream_t)stream));
  return 0;
}
int uwm_resize_threshold_ragged(const float* logits, int ld, int N, int h, int w, const uwm_image_desc* out_descs, float threshold,
                                int apply_sigmoid, uint8_t* mask, size_t mask_bytes, uwm_stream stream) {
  if (!logits || !out_descs || !mask) return fail("uwm_resize_threshold_ragged: null argument");
  if (N < 1 || h < 1 || w < 1 || ld < 1 || mask_bytes < 1)
    return fail("uwm_resize_threshold_ragged: N, h, w, ld and mask_bytes must be >= 1 (got %d, %d, %d, %d, %zu)", N, h, w, ld, mask_bytes);
  if (N > (1 << 24)) return fail("uwm_resize_threshold_ragged: N too large for one launch (%d)", N);
  if ((uintptr_t)out_descs & 7) return fail("uwm_resize_threshold_ragged: descriptors must be 8-byte aligned");
  LCHK(launch_resize_threshold_ragged(logits, ld, N, h, w, (const ImageDesc*)out_descs, threshold, apply_sigmoid, mask, mask_bytes,
                                      (hipStream_t)stream));
  return 0;
}
// ---- masks from watermarked / clean pairs (pair_mask_u8.hip): every argument is checked here, before any launch
int uwm_pair_mask_u8(const uint8_t* wm, size_t wm_bytes, const uwm_image_desc* wm_descs, const uint8_t* clean, size_t clean_bytes,
                     const uwm_image_desc* clean_descs, int N, int C, int threshold, int open, uint8_t* mask, size_t mask_bytes,
                     const uwm_image_desc* mask_descs, uwm_stream stream) {
  if (!wm || !wm_descs || !clean || !clean_descs || !mask || !mask_descs) return fail("uwm_pair_mask_u8: null argument");
  if (C != 3) return fail("uwm_pair_mask_u8: C must be 3 (RGB pairs; got %d)", C);
  if (threshold < 0 || threshold > 255) return fail("uwm_pair_mask_u8: threshold must be 0..255 (got %d)", threshold);
  if (N < 1 || wm_bytes < 1 || clean_bytes < 1 || mask_bytes < 1)
    return fail("uwm_pair_mask_u8: N, wm_bytes, clean_bytes and mask_bytes must be >= 1 (got %d, %zu, %zu, %zu)", N, wm_bytes, clean_bytes, mask_bytes);
  if (N > 2147483647 / kPairMaskBlocks) return fail("uwm_pair_mask_u8: N too large for one launch (%d)", N);
  if (((uintptr_t)wm | (uintptr_t)clean) & 3) return fail("uwm_pair_mask_u8: wm and clean must be 4-byte aligned");
  if (((uintptr_t)wm_descs | (uintptr_t)clean_descs | (uintptr_t)mask_descs) & 7) return fail("uwm_pair_mask_u8: descriptors must be 8-byte aligned");
  LCHK(launch_pair_mask_u8(wm, wm_bytes, (const ImageDesc*)wm_descs, clean, clean_bytes, (const ImageDesc*)clean_descs, N, threshold, open != 0,
                           mask, mask_bytes, (const ImageDesc*)mask_descs, (hipStream_t)stream));
  return 0;
}
// ---- logo-watermarked training samples (synth_u8.hip): every argument is checked here, before any launch (descriptors and jobs are
// device memory: the kernels check each job and skip the ones that do not fit)
static_assert(sizeof(uwm_synth_job) == sizeof(SynthJob) && sizeof(uwm_synth_job) == 488 && offsetof(uwm_synth_job, rot) == 136 &&
              offsetof(uwm_synth_job, opacity) == offsetof(SynthJob, opacity) && offsetof(uwm_synth_job, x) == offsetof(SynthJob, x), "uwm_synth_job layout");
size_t uwm_synth_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps) {
  const size_t b = synth_workspace_bytes(N, K, max_patch_pixels, max_taps);
  if (!b) (void)fail("uwm_synth_workspace_bytes: need N >= 1, K in 1..%d, max_patch_pixels in 1..%lld, max_taps in 1..%lld and N * K * %d within one "
                     "launch (got %d, %d, %lld, %lld)", kSynthMaxSlots, kSynthMaxPatchPixels, kSynthMaxTaps, kSynthBlocks, N, K, max_patch_pixels, max_taps);
  return b;
}
static int synth_args_check(const char* fn, const void* logos, size_t logo_bytes, const void* logo_descs, int num_logos, const void* jobs, int N, int K,
                            long long P, long long T, const void* ws, size_t ws_bytes) {
  if (!logos || !logo_descs || !jobs || !ws) return fail("%s: null argument", fn);
  if (num_logos < 1 || logo_bytes < 1) return fail("%s: num_logos and logo_bytes must be >= 1 (got %d, %zu)", fn, num_logos, logo_bytes);
  const size_t need = synth_workspace_bytes(N, K, P, T);
  if (!need) return fail("%s: need N >= 1, K in 1..%d, max_patch_pixels in 1..%lld, max_taps in 1..%lld and N * K * %d within one launch (got %d, %d, %lld, "
                         "%lld)", fn, kSynthMaxSlots, kSynthMaxPatchPixels, kSynthMaxTaps, kSynthBlocks, N, K, P, T);
  if (ws_bytes < need) return fail("%s: workspace of %zu bytes, need %zu (uwm_synth_workspace_bytes)", fn, ws_bytes, need);
  if ((uintptr_t)logos & 3) return fail("%s: logos must be 4-byte aligned", fn);
  if (((uintptr_t)logo_descs | (uintptr_t)jobs | (uintptr_t)ws) & 7) return fail("%s: descriptors, jobs and workspace must be 8-byte aligned", fn);
  return 0;
}
int uwm_synth_u8(uint8_t* images, size_t image_bytes, const uwm_image_desc* image_descs, uint8_t* masks, size_t mask_bytes,
                 const uwm_image_desc* mask_descs, const uint8_t* logos, size_t logo_bytes, const uwm_image_desc* logo_descs, int num_logos,
                 const uwm_synth_job* jobs, int N, int K, long long max_patch_pixels, long long max_taps, void* ws, size_t ws_bytes,
                 uwm_stream stream) {
  if (!images || !image_descs) return fail("uwm_synth_u8: null argument");
  if (synth_args_check("uwm_synth_u8", logos, logo_bytes, logo_descs, num_logos, jobs, N, K, max_patch_pixels, max_taps, ws, ws_bytes)) return 1;
  if (image_bytes < 1) return fail("uwm_synth_u8: image_bytes must be >= 1");
  if ((uintptr_t)image_descs & 7) return fail("uwm_synth_u8: descriptors must be 8-byte aligned");
  if (masks && (!mask_descs || mask_bytes < 1 || ((uintptr_t)mask_descs & 7)))
    return fail("uwm_synth_u8: masks need mask_descs (8-byte aligned) and mask_bytes >= 1");
  LCHK(launch_synth_u8(images, image_bytes, (const ImageDesc*)image_descs, masks, mask_bytes, (const ImageDesc*)mask_descs, logos, logo_bytes,
                       (const ImageDesc*)logo_descs, num_logos, (const SynthJob*)jobs, N, K, max_patch_pixels, max_taps, ws, ws_bytes,
                       (hipStream_t)stream));
  return 0;
}
int uwm_op_synth_patches(const uint8_t* logos, size_t logo_bytes, const uwm_image_desc* logo_descs, int num_logos, const uwm_synth_job* jobs, int J,
                         long long max_patch_pixels, long long max_taps, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes,
                         uwm_stream stream) {
  if (!out) return fail("uwm_op_synth_patches: null argument");
  if (synth_args_check("uwm_op_synth_patches", logos, logo_bytes, logo_descs, num_logos, jobs, J, 1, max_patch_pixels, max_taps, ws, ws_bytes)) return 1;
  if ((uintptr_t)out & 3) return fail("uwm_op_synth_patches: out must be 4-byte aligned");
  if (out_bytes / 4 / (size_t)max_patch_pixels < (size_t)J)
    return fail("uwm_op_synth_patches: out of %zu bytes, need J * max_patch_pixels * 4 = %zu", out_bytes, (size_t)J * (size_t)max_patch_pixels * 4);
  LCHK(launch_synth_patches(logos, logo_bytes, (const ImageDesc*)logo_descs, num_logos, (const SynthJob*)jobs, J, max_patch_pixels, max_taps, ws,
                            ws_bytes, out, out_bytes, (hipStream_t)stream));
  return 0;
}
int uwm_lanczos_table_ints(int in, int out) {
  if (in < 1 || out < 1 || in > 32767 || out > 32767) return 0;
  return out * (synth_lanczos_ksize(in, out) + 2);
}
int uwm_op_lanczos_table(int in, int out, int* table, size_t table_ints, uwm_stream stream) {
  if (!table) return fail("uwm_op_lanczos_table: null argument");
  if (in < 1 || out < 1 || in > 32767 || out > 32767) return fail("uwm_op_lanczos_table: in and out must be 1..32767 (got %d, %d)", in, out);
  if ((uintptr_t)table & 3) return fail("uwm_op_lanczos_table: table must be 4-byte aligned");
  if (table_ints < (size_t)uwm_lanczos_table_ints(in, out))
    return fail("uwm_op_lanczos_table: table of %zu ints, need %d (uwm_lanczos_table_ints)", table_ints, uwm_lanczos_table_ints(in, out));
  LCHK(launch_lanczos_table(in, out, table, (hipStream_t)stream));
  return 0;
}
// ---- text-watermarked training samples (synth_text_u8.hip): checked as the logo entries are
static_assert(sizeof(uwm_text_job) == sizeof(TextJob) && sizeof(uwm_text_job) == 416 && offsetof(uwm_text_job, rot) == 112 &&
              offsetof(uwm_text_job, opacity) == offsetof(TextJob, opacity) && offsetof(uwm_text_job, x) == offsetof(TextJob, x) &&
              offsetof(uwm_text_job, fit) == offsetof(TextJob, fit), "uwm_text_job layout");
size_t uwm_synth_text_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps) {
  const size_t b = synth_text_workspace_bytes(N, K, max_patch_pixels, max_taps);
  if (!b) (void)fail("uwm_synth_text_workspace_bytes: need N >= 1, K in 1..%d, max_patch_pixels in 1..%lld, max_taps in 1..%lld and N * K * %d within "
                     "one launch (got %d, %d, %lld, %lld)", kSynthMaxSlots, kSynthMaxPatchPixels, kSynthMaxTaps, kSynthBlocks, N, K, max_patch_pixels, max_taps);
  return b;
}
static int text_args_check(const char* fn, const void* planes, size_t plane_bytes, const void* plane_descs, int num_planes, const void* jobs, int N,
                           int K, long long P, long long T, const void* ws, size_t ws_bytes) {
  if (!planes || !plane_descs || !jobs || !ws) return fail("%s: null argument", fn);
  if (num_planes < 1 || plane_bytes < 1) return fail("%s: num_planes and plane_bytes must be >= 1 (got %d, %zu)", fn, num_planes, plane_bytes);
  const size_t need = synth_text_workspace_bytes(N, K, P, T);
  if (!need) return fail("%s: need N >= 1, K in 1..%d, max_patch_pixels in 1..%lld, max_taps in 1..%lld and N * K * %d within one launch (got %d, %d, %lld, "
                         "%lld)", fn, kSynthMaxSlots, kSynthMaxPatchPixels, kSynthMaxTaps, kSynthBlocks, N, K, P, T);
  if (ws_bytes < need) return fail("%s: workspace of %zu bytes, need %zu (uwm_synth_text_workspace_bytes)", fn, ws_bytes, need);
  if ((uintptr_t)planes & 3) return fail("%s: planes must be 4-byte aligned", fn);
  if (((uintptr_t)plane_descs | (uintptr_t)jobs | (uintptr_t)ws) & 7) return fail("%s: descriptors, jobs and workspace must be 8-byte aligned", fn);
  return 0;
}
int uwm_synth_text_u8(uint8_t* images, size_t image_bytes, const uwm_image_desc* image_descs, uint8_t* masks, size_t mask_bytes,
                      const uwm_image_desc* mask_descs, int mask_mode, const uint8_t* planes, size_t plane_bytes,
                      const uwm_image_desc* plane_descs, int num_planes, const uwm_text_job* jobs, int N, int K, long long max_patch_pixels,
                      long long max_taps, void* ws, size_t ws_bytes, uwm_stream stream) {
  if (!images || !image_descs) return fail("uwm_synth_text_u8: null argument");
  if (text_args_check("uwm_synth_text_u8", planes, plane_bytes, plane_descs, num_planes, jobs, N, K, max_patch_pixels, max_taps, ws, ws_bytes)) return 1;
  if (image_bytes < 1) return fail("uwm_synth_text_u8: image_bytes must be >= 1");
  if ((uintptr_t)image_descs & 7) return fail("uwm_synth_text_u8: descriptors must be 8-byte aligned");
  if (mask_mode != 0 && mask_mode != 1) return fail("uwm_synth_text_u8: mask_mode must be 0 (paste) or 1 (mixed) (got %d)", mask_mode);
  if (masks && (!mask_descs || mask_bytes < 1 || ((uintptr_t)mask_descs & 7)))
    return fail("uwm_synth_text_u8: masks need mask_descs (8-byte aligned) and mask_bytes >= 1");
  LCHK(launch_synth_text_u8(images, image_bytes, (const ImageDesc*)image_descs, masks, mask_bytes, (const ImageDesc*)mask_descs, mask_mode, planes,
                            plane_bytes, (const ImageDesc*)plane_descs, num_planes, (const TextJob*)jobs, N, K, max_patch_pixels, max_taps, ws,
                            ws_bytes, (hipStream_t)stream));
  return 0;
}
int uwm_op_text_patches(const uint8_t* planes, size_t plane_bytes, const uwm_image_desc* plane_descs, int num_planes, const uwm_text_job* jobs, int J,
                        long long max_patch_pixels, long long max_taps, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes,
                        uwm_stream stream) {
  if (!out) return fail("uwm_op_text_patches: null argument");
  if (text_args_check("uwm_op_text_patches", planes, plane_bytes, plane_descs, num_planes, jobs, J, 1, max_patch_pixels, max_taps, ws, ws_bytes)) return 1;
  if ((uintptr_t)out & 3) return fail("uwm_op_text_patches: out must be 4-byte aligned");
  if (out_bytes / 4 / (size_t)max_patch_pixels < (size_t)J)
    return fail("uwm_op_text_patches: out of %zu bytes, need J * max_patch_pixels * 4 = %zu", out_bytes, (size_t)J * (size_t)max_patch_pixels * 4);
  LCHK(launch_text_patches(planes, plane_bytes, (const ImageDesc*)plane_descs, num_planes, (const TextJob*)jobs, J, max_patch_pixels, max_taps, ws,
                           ws_bytes, out, out_bytes, (hipStream_t)stream));
  return 0;
}
int uwm_predict_images_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, const float* mean,
                          const float* std, float threshold, int apply_sigmoid, const uwm_image_desc* out_descs, uint8_t* mask,
                          size_t mask_bytes, float* logits, void* ws, size_t ws_bytes, int N, int H, int W, uwm_stream stream) {
  if (!h || !src || !in_descs || !mean || !std || !out_descs || !mask || !ws) return fail("uwm_predict_images_u8: null argument");
  if (check_shape(N, H, W)) return 1;
  if (!h->params || !h->buffers) return fail("uwm_predict_images_u8: call uwm_bind first");
  if (src_bytes < 1 || mask_bytes < 1) return fail("uwm_predict_images_u8: src_bytes and mask_bytes must be >= 1");
  const int C = h->desc.in_channels;
  if (C < 1 || C > 4) return fail("uwm_predict_images_u8: the model takes %d channels; images have 1..4", C);
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_predict_images_u8: std[%d] must be positive", c);
  if ((uintptr_t)src & 3) return fail("uwm_predict_images_u8: src must be 4-byte aligned");
  if (((uintptr_t)in_descs | (uintptr_t)out_descs) & 7) return fail("uwm_predict_images_u8: descriptors must be 8-byte aligned");
  if (((uintptr_t)logits | (uintptr_t)ws) & 15) return fail("uwm_predict_images_u8: logits and workspace must be 16-byte aligned");
  const size_t need = uwm_predict_workspace_bytes(h, N, H, W, logits ? 0 : 1);
  if (ws_bytes < need) return fail("uwm_predict_images_u8: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  float* lg = logits ? logits : (float*)ws + h->plan.bytes / sizeof(float);      // (no caller buffer: behind the plan)
  h->have_fwd = false;
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  LCHK(launch_resize_norm_u8_nhwc4(src, src_bytes, (const ImageDesc*)in_descs, N, C, H, W, mean, std, (float*)ws + h->plan.x4, st));
  if (do_forward(h, nullptr, lg, (float*)ws, N, H, W, 0, st)) return 1;
  LCHK(launch_resize_threshold_ragged(lg, h->CP, N, H, W, (const ImageDesc*)out_descs, threshold, apply_sigmoid, mask, mask_bytes, st));
  return 0;
}
// ---- prediction at native resolution (tile_u8.hip): every argument is checked here, before any launch (the tile table, the plans and
// the descriptors are device memory: the kernels check them)
static_assert(sizeof(uwm_tile_desc) == sizeof(TileDesc) && sizeof(uwm_tile_desc) == 16 && offsetof(uwm_tile_desc, first) == offsetof(TileDesc, first) &&
              sizeof(uwm_tile_image) == sizeof(TileImage) && sizeof(uwm_tile_image) == 16 && offsetof(uwm_tile_image, nx) == offsetof(TileImage, nx),
              "uwm_tile_desc / uwm_tile_image layout");
static int tile_shape_check(const char* fn, int K, int T_h, int T_w, int overlap) {
  if (K < 1) return fail("%s: K must be >= 1 (got %d)", fn, K);
  if (T_h < 1 || T_w < 1 || T_h > kTileMaxSide || T_w > kTileMaxSide) return fail("%s: tile sides must be 1..%d (got %d x %d)", fn, kTileMaxSide, T_h, T_w);
  if (overlap < 0 || 2 * overlap > (T_h < T_w ? T_h : T_w)) return fail("%s: overlap must lie in [0, T / 2] on both axes (tile %d x %d, got %d)", fn, T_h, T_w, overlap);
  if ((long long)K * ((T_h + kTileRowsPerBlock - 1) / kTileRowsPerBlock) > 2147483647ll) return fail("%s: K * T_h too large for one launch (%d x %d)", fn, K, T_h);
  return 0;
}
int uwm_op_tile_norm_u8_nhwc4(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int num_images, const uwm_tile_desc* tiles, int K,
                              int C, int T_h, int T_w, const float* mean, const float* std, float* out, uwm_stream stream) {
  if (!src || !descs || !tiles || !mean || !std || !out) return fail("uwm_op_tile_norm_u8_nhwc4: null argument");
  if (tile_shape_check("uwm_op_tile_norm_u8_nhwc4", K, T_h, T_w, 0)) return 1;
  if (C < 1 || C > 4) return fail("uwm_op_tile_norm_u8_nhwc4: C must be 1..4 (got %d)", C);
  if (num_images < 1 || src_bytes < 1) return fail("uwm_op_tile_norm_u8_nhwc4: num_images and src_bytes must be >= 1 (got %d, %zu)", num_images, src_bytes);
  if ((uintptr_t)src & 3) return fail("uwm_op_tile_norm_u8_nhwc4: src must be 4-byte aligned");
  if (((uintptr_t)descs & 7) || ((uintptr_t)tiles & 3)) return fail("uwm_op_tile_norm_u8_nhwc4: descriptors must be 8-byte, tiles 4-byte aligned");
  if ((uintptr_t)out & 15) return fail("uwm_op_tile_norm_u8_nhwc4: out must be 16-byte aligned");
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_op_tile_norm_u8_nhwc4: std[%d] must be positive", c);
  LCHK(launch_tile_norm_u8_nhwc4(src, src_bytes, (const ImageDesc*)descs, num_images, (const TileDesc*)tiles, K, C, T_h, T_w, mean, std, out,
                                 (hipStream_t)stream));
  return 0;
}
static int tile_blend_args_check(const char* fn, int K, const void* plans, int num_images, int T_h, int T_w, int overlap, const void* in_descs,
                                 int C, const void* out_descs, float threshold, const void* mask, size_t mask_bytes, const void* logits_out) {
  if (!plans || !out_descs || !mask) return fail("%s: null argument", fn);
  if (tile_shape_check(fn, K, T_h, T_w, overlap)) return 1;
  if (num_images < 1 || mask_bytes < 1) return fail("%s: num_images and mask_bytes must be >= 1 (got %d, %zu)", fn, num_images, mask_bytes);
  if (num_images > 2147483647 / kTileBlendBlocks) return fail("%s: too many images for one launch (%d)", fn, num_images);
  if (!std::isfinite(threshold)) return fail("%s: threshold must be finite", fn);
  if (in_descs && (C < 1 || C > 4)) return fail("%s: C must be 1..4 (got %d)", fn, C);
  if (((uintptr_t)in_descs | (uintptr_t)out_descs) & 7) return fail("%s: descriptors must be 8-byte aligned", fn);
  if (((uintptr_t)plans | (uintptr_t)logits_out) & 3) return fail("%s: plans and logits_out must be 4-byte aligned", fn);
  return 0;
}
int uwm_tile_blend_threshold_ragged(const float* tile_logits, int K, const uwm_tile_image* plans, int num_images, int T_h, int T_w, int overlap,
                                    const uwm_image_desc* in_descs, size_t src_bytes, int C, const uwm_image_desc* out_descs, float threshold,
                                    int apply_sigmoid, uint8_t* mask, size_t mask_bytes, float* logits_out, uwm_stream stream) {
  if (!tile_logits) return fail("uwm_tile_blend_threshold_ragged: null argument");
  if ((uintptr_t)tile_logits & 3) return fail("uwm_tile_blend_threshold_ragged: tile_logits must be 4-byte aligned");
  if (tile_blend_args_check("uwm_tile_blend_threshold_ragged", K, plans, num_images, T_h, T_w, overlap, in_descs, C, out_descs, threshold, mask,
                            mask_bytes, logits_out))
    return 1;
  LCHK(launch_tile_blend_threshold_ragged(tile_logits, K, (const TileImage*)plans, num_images, T_h, T_w, overlap, (const ImageDesc*)in_descs, src_bytes,
                                          C, (const ImageDesc*)out_descs, threshold, apply_sigmoid, mask, mask_bytes, logits_out, (hipStream_t)stream));
  return 0;
}
// the workspace of uwm_predict_tiled_u8: the eval plan of (N, T_h, T_w) with the forward's logits behind it, then (256-byte aligned)
// the tile-logit store [K][T_h][T_w], which is the workspace's tail
size_t uwm_predict_tiled_workspace_bytes(uwm_handle h, int N, int K, int T_h, int T_w) {
  if (K < 1 || T_h < 1 || T_w < 1) { (void)fail("uwm_predict_tiled_workspace_bytes: K and the tile sides must be >= 1 (got %d, %d x %d)", K, T_h, T_w); return 0; }
  const size_t fwd = uwm_predict_workspace_bytes(h, N, T_h, T_w, 1);
  if (!fwd) return 0;
  return ((fwd + 255) & ~(size_t)255) + (size_t)K * T_h * T_w * sizeof(float);
}
int uwm_predict_tiled_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, int num_images,
                         const uwm_tile_desc* tiles, int K, const uwm_tile_image* plans, int T_h, int T_w, int overlap, const float* mean,
                         const float* std, float threshold, int apply_sigmoid, const uwm_image_desc* out_descs, uint8_t* mask, size_t mask_bytes,
                         float* logits_out, void* ws, size_t ws_bytes, int N, uwm_stream stream) {
  if (!h || !src || !in_descs || !tiles || !mean || !std || !ws) return fail("uwm_predict_tiled_u8: null argument");
  if (check_shape(N, T_h, T_w)) return 1;
  if (tile_blend_args_check("uwm_predict_tiled_u8", K, plans, num_images, T_h, T_w, overlap, in_descs, h->desc.in_channels, out_descs, threshold, mask,
                            mask_bytes, logits_out))
    return 1;
  if (K % N) return fail("uwm_predict_tiled_u8: K must be a multiple of the forward batch N (got %d, %d)", K, N);
  if (!h->params || !h->buffers) return fail("uwm_predict_tiled_u8: call uwm_bind first");
  if (src_bytes < 1) return fail("uwm_predict_tiled_u8: src_bytes must be >= 1");
  const int C = h->desc.in_channels;
  if (C < 1 || C > 4) return fail("uwm_predict_tiled_u8: the model takes %d channels; images have 1..4", C);
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_predict_tiled_u8: std[%d] must be positive", c);
  if ((uintptr_t)src & 3) return fail("uwm_predict_tiled_u8: src must be 4-byte aligned");
  if ((uintptr_t)tiles & 3) return fail("uwm_predict_tiled_u8: tiles must be 4-byte aligned");
  if ((uintptr_t)ws & 15) return fail("uwm_predict_tiled_u8: workspace must be 16-byte aligned");
  const size_t need = uwm_predict_tiled_workspace_bytes(h, N, K, T_h, T_w);      // (also plans the eval forward of (N, T_h, T_w))
  if (!need) return 1;
  if (ws_bytes < need) return fail("uwm_predict_tiled_u8: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  const size_t plane = (size_t)T_h * T_w;
  float* lg = (float*)ws + h->plan.bytes / sizeof(float);                        // the forward's logits: behind the plan
  float* store = (float*)((char*)ws + (need - (size_t)K * plane * sizeof(float)));
  h->have_fwd = false;
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  for (int k0 = 0; k0 < K; k0 += N) {
    LCHK(launch_tile_norm_u8_nhwc4(src, src_bytes, (const ImageDesc*)in_descs, num_images, (const TileDesc*)tiles + k0, N, C, T_h, T_w, mean, std,
                                   (float*)ws + h->plan.x4, st));
    if (do_forward(h, nullptr, lg, (float*)ws, N, T_h, T_w, 0, st)) return 1;
    LCHK(launch_tile_store(lg, h->CP, (size_t)N * plane, store + (size_t)k0 * plane, st));
  }
  LCHK(launch_tile_blend_threshold_ragged(store, K, (const TileImage*)plans, num_images, T_h, T_w, overlap, (const ImageDesc*)in_descs, src_bytes, C,
                                          (const ImageDesc*)out_descs, threshold, apply_sigmoid, mask, mask_bytes, logits_out, st));
  return 0;
}
// ---- test-time augmentation (tta.hip): every argument is checked here, before any launch
static int view_count(int views) { int k = 0; for (int c = 0; c < 8; ++c) k += (views >> c) & 1; return k; }
static int view_set_check(const char* fn, int views, int H, int W) {
  if (views < 1 || views > 255) return fail("%s: views must be 1..255 (got %d)", fn, views);
  if ((views & 0xAA) && H != W) return fail("%s: a quarter-turn view (codes 1, 3, 5, 7) needs H == W (views 0x%02x, got %d x %d)", fn, views, H, W);
  return 0;
}
static int view_range_check(const char* fn, int views, int H, int W, int slot0, int num_slots, int num_items) {
  if (view_set_check(fn, views, H, W)) return 1;
  if (H < 1 || W < 1) return fail("%s: H and W must be >= 1 (got %d x %d)", fn, H, W);
  if (slot0 < 0 || num_slots < 1 || num_items < 1) return fail("%s: slot0 must be >= 0, num_slots and the item count >= 1 (got %d, %d, %d)", fn, slot0, num_slots, num_items);
  if ((long long)slot0 + num_slots > 2147483647ll || (long long)num_items * view_count(views) + num_slots > 2147483647ll)
    return fail("%s: slot range overflows (slot0 %d, num_slots %d, %d items of %d views)", fn, slot0, num_slots, num_items, view_count(views));
  if ((long long)num_slots * ((H + 15) / 16) * ((W + 15) / 16) > 2147483647ll) return fail("%s: num_slots * H * W too large for one launch (%d x %d x %d)", fn, num_slots, H, W);
  return 0;
}
size_t uwm_view_stage_bytes(int views, int num_slots, int H, int W) {
  if (view_set_check("uwm_view_stage_bytes", views, H, W)) return 0;
  if (num_slots < 1 || H < 1 || W < 1) { (void)fail("uwm_view_stage_bytes: num_slots, H and W must be >= 1 (got %d, %d, %d)", num_slots, H, W); return 0; }
  return (size_t)view_stage_planes(views, num_slots) * H * W * 4 * sizeof(float);
}
static int view_stage_check(const char* fn, int views, int num_slots, int H, int W, const void* stage, size_t stage_bytes, const void* out) {
  if (!stage || !out) return fail("%s: null argument", fn);
  if (((uintptr_t)stage | (uintptr_t)out) & 15) return fail("%s: stage and out must be 16-byte aligned", fn);
  const size_t need = uwm_view_stage_bytes(views, num_slots, H, W);
  if (stage_bytes < need) return fail("%s: stage too small (%zu < %zu bytes, uwm_view_stage_bytes)", fn, stage_bytes, need);
  return 0;
}
int uwm_op_resize_norm_view_u8_nhwc4(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int num_images, int C, int H, int W,
                                     const float* mean, const float* std, int views, int slot0, int num_slots, float* stage, size_t stage_bytes,
                                     float* out, uwm_stream stream) {
  const char* fn = "uwm_op_resize_norm_view_u8_nhwc4";
  if (!mean || !std) return fail("%s: null argument", fn);
  if (resize_args_check(fn, src, src_bytes, descs, num_images, C, H, W, out)) return 1;
  if (view_range_check(fn, views, H, W, slot0, num_slots, num_images)) return 1;
  if (view_stage_check(fn, views, num_slots, H, W, stage, stage_bytes, out)) return 1;
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("%s: std[%d] must be positive", fn, c);
  LCHK(launch_resize_norm_view_u8_nhwc4(src, src_bytes, (const ImageDesc*)descs, num_images, C, H, W, mean, std, views, slot0, num_slots, stage, out,
                                        (hipStream_t)stream));
  return 0;
}
int uwm_op_tile_norm_view_u8_nhwc4(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int num_images, const uwm_tile_desc* tiles, int K,
                                   int C, int T_h, int T_w, const float* mean, const float* std, int views, int slot0, int num_slots, float* stage,
                                   size_t stage_bytes, float* out, uwm_stream stream) {
  const char* fn = "uwm_op_tile_norm_view_u8_nhwc4";
  if (!src || !descs || !tiles || !mean || !std) return fail("%s: null argument", fn);
  if (tile_shape_check(fn, K, T_h, T_w, 0)) return 1;
  if (C < 1 || C > 4) return fail("%s: C must be 1..4 (got %d)", fn, C);
  if (num_images < 1 || src_bytes < 1) return fail("%s: num_images and src_bytes must be >= 1 (got %d, %zu)", fn, num_images, src_bytes);
  if (view_range_check(fn, views, T_h, T_w, slot0, num_slots, K)) return 1;
  if (view_stage_check(fn, views, num_slots, T_h, T_w, stage, stage_bytes, out)) return 1;
  if ((uintptr_t)src & 3) return fail("%s: src must be 4-byte aligned", fn);
  if (((uintptr_t)descs & 7) || ((uintptr_t)tiles & 3)) return fail("%s: descriptors must be 8-byte, tiles 4-byte aligned", fn);
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("%s: std[%d] must be positive", fn, c);
  LCHK(launch_tile_norm_view_u8_nhwc4(src, src_bytes, (const ImageDesc*)descs, num_images, (const TileDesc*)tiles, K, C, T_h, T_w, mean, std, views,
                                      slot0, num_slots, stage, out, (hipStream_t)stream));
  return 0;
}
int uwm_op_view_merge(const float* logits, int ld, int H, int W, int views, int slot0, int num_slots, int num_items, float* store,
                      uwm_stream stream) {
  const char* fn = "uwm_op_view_merge";
  if (!logits || !store) return fail("%s: null argument", fn);
  if (ld < 1) return fail("%s: ld must be >= 1 (got %d)", fn, ld);
  if (view_range_check(fn, views, H, W, slot0, num_slots, num_items)) return 1;
  if (((uintptr_t)logits | (uintptr_t)store) & 3) return fail("%s: logits and store must be 4-byte aligned", fn);
  LCHK(launch_view_merge(logits, ld, H, W, views, slot0, num_slots, num_items, store, (hipStream_t)stream));
  return 0;
}
// the workspace of the two model-level calls: the eval plan of (N, H, W) with the forward's logits behind it, then (256-byte aligned) the
// staging planes of one chunk, then (256-byte aligned) the merged store [items][H][W], which is the workspace's tail
static size_t tta_workspace_bytes(const char* fn, uwm_handle h, int N, int H, int W, int items, int views) {
  if (!h) { (void)fail("%s: null argument", fn); return 0; }
  if (view_set_check(fn, views, H, W)) return 0;
  if (items < 1) { (void)fail("%s: the item count must be >= 1 (got %d)", fn, items); return 0; }
  const size_t fwd = uwm_predict_workspace_bytes(h, N, H, W, 1);
  if (!fwd) return 0;
  const size_t stage = (size_t)view_stage_planes(views, N) * H * W * 4 * sizeof(float);
  return ((fwd + 255) & ~(size_t)255) + ((stage + 255) & ~(size_t)255) + (size_t)items * H * W * sizeof(float);
}
size_t uwm_predict_images_tta_workspace_bytes(uwm_handle h, int N, int H, int W, int num_images, int views) {
  return tta_workspace_bytes("uwm_predict_images_tta_workspace_bytes", h, N, H, W, num_images, views);
}
size_t uwm_predict_tiled_tta_workspace_bytes(uwm_handle h, int N, int K, int T_h, int T_w, int views) {
  return tta_workspace_bytes("uwm_predict_tiled_tta_workspace_bytes", h, N, T_h, T_w, K, views);
}
int uwm_predict_images_tta_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, int num_images, int views,
                              const float* mean, const float* std, float threshold, int apply_sigmoid, const uwm_image_desc* out_descs,
                              uint8_t* mask, size_t mask_bytes, float* merged, void* ws, size_t ws_bytes, int N, int H, int W, uwm_stream stream) {
  const char* fn = "uwm_predict_images_tta_u8";
  if (!h || !src || !in_descs || !mean || !std || !out_descs || !mask || !ws) return fail("%s: null argument", fn);
  if (check_shape(N, H, W)) return 1;
  if (view_range_check(fn, views, H, W, 0, N, num_images)) return 1;
  if (num_images > (1 << 24)) return fail("%s: too many images for one launch (%d)", fn, num_images);
  if (src_bytes < 1 || mask_bytes < 1) return fail("%s: src_bytes and mask_bytes must be >= 1", fn);
  if (!std::isfinite(threshold)) return fail("%s: threshold must be finite", fn);
  const int C = h->desc.in_channels;
  if (C < 1 || C > 4) return fail("%s: the model takes %d channels; images have 1..4", fn, C);
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("%s: std[%d] must be positive", fn, c);
  if ((uintptr_t)src & 3) return fail("%s: src must be 4-byte aligned", fn);
  if (((uintptr_t)in_descs | (uintptr_t)out_descs) & 7) return fail("%s: descriptors must be 8-byte aligned", fn);
  if ((uintptr_t)ws & 15) return fail("%s: workspace must be 16-byte aligned", fn);
  if ((uintptr_t)merged & 3) return fail("%s: merged must be 4-byte aligned", fn);
  if (!h->params || !h->buffers) return fail("%s: call uwm_bind first", fn);
  const size_t need = uwm_predict_images_tta_workspace_bytes(h, N, H, W, num_images, views);      // (also plans the eval forward of (N, H, W))
  if (!need) return 1;
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  const size_t plane = (size_t)H * W, store_bytes = (size_t)num_images * plane * sizeof(float);
  const size_t stage_bytes = ((size_t)view_stage_planes(views, N) * plane * 4 * sizeof(float) + 255) & ~(size_t)255;
  float* lg = (float*)ws + h->plan.bytes / sizeof(float);                        // the forward's logits: behind the plan
  float* stage = (float*)((char*)ws + (need - store_bytes - stage_bytes));
  float* store = merged ? merged : (float*)((char*)ws + (need - store_bytes));
  const long long slots = (long long)num_images * view_count(views);
  h->have_fwd = false;
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  for (long long s0 = 0; s0 < slots; s0 += N) {
    LCHK(launch_resize_norm_view_u8_nhwc4(src, src_bytes, (const ImageDesc*)in_descs, num_images, C, H, W, mean, std, views, (int)s0, N, stage,
                                          (float*)ws + h->plan.x4, st));
    if (do_forward(h, nullptr, lg, (float*)ws, N, H, W, 0, st)) return 1;
    LCHK(launch_view_merge(lg, h->CP, H, W, views, (int)s0, N, num_images, store, st));
  }
  LCHK(launch_resize_threshold_ragged(store, 1, num_images, H, W, (const ImageDesc*)out_descs, threshold, apply_sigmoid, mask, mask_bytes, st));
  return 0;
}
int uwm_predict_tiled_tta_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, int num_images,
                             const uwm_tile_desc* tiles, int K, const uwm_tile_image* plans, int T_h, int T_w, int overlap, const float* mean,
                             const float* std, float threshold, int apply_sigmoid, const uwm_image_desc* out_descs, uint8_t* mask, size_t mask_bytes,
                             float* logits_out, void* ws, size_t ws_bytes, int N, int views, uwm_stream stream) {
  const char* fn = "uwm_predict_tiled_tta_u8";
  if (!h || !src || !in_descs || !tiles || !mean || !std || !ws) return fail("%s: null argument", fn);
  if (check_shape(N, T_h, T_w)) return 1;
  if (tile_blend_args_check(fn, K, plans, num_images, T_h, T_w, overlap, in_descs, h->desc.in_channels, out_descs, threshold, mask, mask_bytes,
                            logits_out))
    return 1;
  if (view_range_check(fn, views, T_h, T_w, 0, N, K)) return 1;
  if (src_bytes < 1) return fail("%s: src_bytes must be >= 1", fn);
  const int C = h->desc.in_channels;
  if (C < 1 || C > 4) return fail("%s: the model takes %d channels; images have 1..4", fn, C);
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("%s: std[%d] must be positive", fn, c);
  if ((uintptr_t)src & 3) return fail("%s: src must be 4-byte aligned", fn);
  if ((uintptr_t)tiles & 3) return fail("%s: tiles must be 4-byte aligned", fn);
  if ((uintptr_t)ws & 15) return fail("%s: workspace must be 16-byte aligned", fn);
  if (!h->params || !h->buffers) return fail("%s: call uwm_bind first", fn);
  const size_t need = uwm_predict_tiled_tta_workspace_bytes(h, N, K, T_h, T_w, views);      // (also plans the eval forward of (N, T_h, T_w))
  if (!need) return 1;
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  const size_t plane = (size_t)T_h * T_w, store_bytes = (size_t)K * plane * sizeof(float);
  const size_t stage_bytes = ((size_t)view_stage_planes(views, N) * plane * 4 * sizeof(float) + 255) & ~(size_t)255;
  float* lg = (float*)ws + h->plan.bytes / sizeof(float);
  float* stage = (float*)((char*)ws + (need - store_bytes - stage_bytes));
  float* store = (float*)((char*)ws + (need - store_bytes));
  const long long slots = (long long)K * view_count(views);
  h->have_fwd = false;
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  for (long long s0 = 0; s0 < slots; s0 += N) {
    LCHK(launch_tile_norm_view_u8_nhwc4(src, src_bytes, (const ImageDesc*)in_descs, num_images, (const TileDesc*)tiles, K, C, T_h, T_w, mean, std,
                                        views, (int)s0, N, stage, (float*)ws + h->plan.x4, st));
    if (do_forward(h, nullptr, lg, (float*)ws, N, T_h, T_w, 0, st)) return 1;
    LCHK(launch_view_merge(lg, h->CP, T_h, T_w, views, (int)s0, N, K, store, st));
  }
  LCHK(launch_tile_blend_threshold_ragged(store, K, (const TileImage*)plans, num_images, T_h, T_w, overlap, (const ImageDesc*)in_descs, src_bytes, C,
                                          (const ImageDesc*)out_descs, threshold, apply_sigmoid, mask, mask_bytes, logits_out, st));
  return 0;
}
// ---- the dataset filter (filter_u8.hip): every argument is checked here, before any launch
size_t uwm_filter_workspace_bytes(int N) {
  const size_t need = filter_workspace_bytes(N);
  if (!need) fail("uwm_filter_workspace_bytes: N must be 1..%d (got %d)", 2147483647 / kFilterBlocks, N);
  return need;
}
static int filter_args_check(const char* fn, int N, const void* out_descs, float threshold, const void* mask, size_t mask_bytes,
                             const void* counts, const void* fws, size_t fws_bytes) {
  if (!out_descs || !counts || !fws) return fail("%s: null argument", fn);
  if (N < 1) return fail("%s: N must be >= 1 (got %d)", fn, N);
  if (N > 2147483647 / kFilterBlocks) return fail("%s: N too large for one launch (%d)", fn, N);
  if (!std::isfinite(threshold)) return fail("%s: threshold must be finite", fn);
  if (mask && mask_bytes < 1) return fail("%s: mask_bytes must be >= 1 with a mask", fn);
  if (((uintptr_t)out_descs | (uintptr_t)counts | (uintptr_t)fws) & 7) return fail("%s: descriptors, counts and the filter workspace must be 8-byte aligned", fn);
  const size_t need = filter_workspace_bytes(N);
  if (fws_bytes < need) return fail("%s: filter workspace too small (%zu < %zu bytes)", fn, fws_bytes, need);
  return 0;
}
int uwm_prob_mask_count_ragged(const float* logits, int ld, int N, int h, int w, const uwm_image_desc* out_descs, float threshold,
                               int post_process, uint8_t* mask, size_t mask_bytes, long long* counts, void* workspace,
                               size_t workspace_bytes, uwm_stream stream) {
  if (!logits) return fail("uwm_prob_mask_count_ragged: null argument");
  if (filter_args_check("uwm_prob_mask_count_ragged", N, out_descs, threshold, mask, mask_bytes, counts, workspace, workspace_bytes)) return 1;
  if (h < 1 || w < 1 || ld < 1) return fail("uwm_prob_mask_count_ragged: h, w and ld must be >= 1 (got %d, %d, %d)", h, w, ld);
  if ((uintptr_t)logits & 3) return fail("uwm_prob_mask_count_ragged: logits must be 4-byte aligned");
  LCHK(launch_prob_mask_count(logits, ld, N, h, w, (const ImageDesc*)out_descs, threshold, post_process != 0, mask, mask_bytes, counts,
                              workspace, workspace_bytes, (hipStream_t)stream));
  return 0;
}
int uwm_filter_images_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, const float* mean,
                         const float* std, float threshold, int post_process, const uwm_image_desc* out_descs, uint8_t* mask,
                         size_t mask_bytes, long long* counts, float* logits, void* ws, size_t ws_bytes, void* fws, size_t fws_bytes,
                         int N, int H, int W, uwm_stream stream) {
  if (!h || !src || !in_descs || !mean || !std || !ws) return fail("uwm_filter_images_u8: null argument");
  if (filter_args_check("uwm_filter_images_u8", N, out_descs, threshold, mask, mask_bytes, counts, fws, fws_bytes)) return 1;
  if (check_shape(N, H, W)) return 1;
  if (!h->params || !h->buffers) return fail("uwm_filter_images_u8: call uwm_bind first");
  if (src_bytes < 1) return fail("uwm_filter_images_u8: src_bytes must be >= 1");
  const int C = h->desc.in_channels;
  if (C < 1 || C > 4) return fail("uwm_filter_images_u8: the model takes %d channels; images have 1..4", C);
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_filter_images_u8: std[%d] must be positive", c);
  if ((uintptr_t)src & 3) return fail("uwm_filter_images_u8: src must be 4-byte aligned");
  if ((uintptr_t)in_descs & 7) return fail("uwm_filter_images_u8: descriptors must be 8-byte aligned");
  if (((uintptr_t)logits | (uintptr_t)ws) & 15) return fail("uwm_filter_images_u8: logits and workspace must be 16-byte aligned");
  const size_t need = uwm_predict_workspace_bytes(h, N, H, W, logits ? 0 : 1);
  if (ws_bytes < need) return fail("uwm_filter_images_u8: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  float* lg = logits ? logits : (float*)ws + h->plan.bytes / sizeof(float);      // (no caller buffer: behind the plan)
  h->have_fwd = false;
  DeviceGuard guard(h->device);
  hipStream_t st = (hipStream_t)stream;
  LCHK(launch_resize_norm_u8_nhwc4(src, src_bytes, (const ImageDesc*)in_descs, N, C, H, W, mean, std, (float*)ws + h->plan.x4, st));
  if (do_forward(h, nullptr, lg, (float*)ws, N, H, W, 0, st)) return 1;
  LCHK(launch_prob_mask_count(lg, h->CP, N, H, W, (const ImageDesc*)out_descs, threshold, post_process != 0, mask, mask_bytes, counts, fws,
                              fws_bytes, st));
  return 0;
}
int uwm_op_preprocess_u8_nhwc4(const uint8_t* images, long long npix, int C, const float* mean, const float* std, float* out,
                               uwm_stream stream) {
  if (!images || !mean || !std || !out || npix < 1 || C < 1 || C > 4) return fail("uwm_op_preprocess_u8_nhwc4: bad argument");
  if (((uintptr_t)images & 3) || ((uintptr_t)out & 15)) return fail("uwm_op_preprocess_u8_nhwc4: images must be 4-byte, out 16-byte aligned");
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_op_preprocess_u8_nhwc4: std[%d] must be positive", c);
  LCHK(launch_preprocess_u8_nhwc4(images, (size_t)npix, C, mean, std, out, (hipStream_t)stream));
  return 0;
}

int uwm_backward(uwm_handle h, const float* dlogits, void* ws, int sb, int se, uwm_stream stream) {
  if (!h || !dlogits || !ws) return fail("uwm_backward: null argument");
  if (!h->grads) return fail("uwm_backward: no gradient arena bound");
  if (!h->have_fwd) return fail("uwm_backward: no training-mode forward is held in the workspace");
  if (sb < 0 || se > h->nstages || sb >= se) return fail("uwm_backward: bad stage range [%d,%d)", sb, se);
  DeviceGuard guard(h->device);
  return do_backward(h, dlogits, (float*)ws, sb, se, (hipStream_t)stream);
}

int uwm_loss(const float* logits, int ld, const void* target, int tdt, long long npix, float w_dice, float w_bce,
             float smooth, float eps, void* scratch, float* loss_out, float* dlogits, int ldd, float grad_scale,
             uwm_stream stream) {
  if (!logits || !target || !scratch || !loss_out || npix <= 0 || ld < 1) return fail("uwm_loss: bad argument");
  if (tdt < 0 || tdt > 3) return fail("uwm_loss: unsupported target dtype %d", tdt);
  if (dlogits && ldd < 1) return fail("uwm_loss: bad dlogits stride");
  LCHK(launch_loss(logits, ld, target, tdt, (size_t)npix, w_dice, w_bce, smooth, eps, (double*)scratch, loss_out, dlogits,
                   ldd, grad_scale, (hipStream_t)stream));
  return 0;
}
int uwm_loss_sums(const float* logits, int ld, const void* target, int tdt, long long npix, void* scratch, uwm_stream stream) {
  if (!logits || !target || !scratch || npix <= 0 || ld < 1) return fail("uwm_loss_sums: bad argument");
  if (tdt < 0 || tdt > 3) return fail("uwm_loss_sums: unsupported target dtype %d", tdt);
  LCHK(launch_loss_sums(logits, ld, target, tdt, (size_t)npix, (double*)scratch, (hipStream_t)stream));
  return 0;
}
int uwm_loss_apply(const float* logits, int ld, const void* target, int tdt, long long npix, long long npix_total, float w_dice,
                   float w_bce, float smooth, float eps, const void* scratch, float* loss_out, float* dlogits, int ldd,
                   float grad_scale, uwm_stream stream) {
  if (!logits || !target || !scratch || !loss_out || npix <= 0 || npix_total < npix || ld < 1) return fail("uwm_loss_apply: bad argument");
  if (tdt < 0 || tdt > 3) return fail("uwm_loss_apply: unsupported target dtype %d", tdt);
  if (dlogits && ldd < 1) return fail("uwm_loss_apply: bad dlogits stride");
  LCHK(launch_loss_apply(logits, ld, target, tdt, (size_t)npix, (double)npix_total, w_dice, w_bce, smooth, eps, (const double*)scratch,
                         loss_out, dlogits, ldd, grad_scale, (hipStream_t)stream));
  return 0;
}
// the argument checks shared by uwm_loss_ext and its halves (0 = fine); nothing is launched before they pass
static int loss_ext_check(const char* who, const float* logits, int ld, const void* target, int tdt, long long npix,
                          const uwm_loss_spec* q, const void* scratch) {
  if (!logits || !target || !q || !scratch || npix <= 0 || ld < 1) return fail("%s: bad argument", who);
  if (tdt < 0 || tdt > 3) return fail("%s: unsupported target dtype %d", who, tdt);
  if (!(q->tversky_gamma > 0.f)) return fail("%s: tversky_gamma must be positive", who);
  if (!(q->focal_gamma >= 0.f)) return fail("%s: focal_gamma must not be negative", who);
  if (!(q->focal_alpha <= 1.f)) return fail("%s: focal_alpha must be <= 1 (negative: none)", who);
  return 0;
}
int uwm_loss_ext(const float* logits, int ld, const void* target, int tdt, long long npix, const uwm_loss_spec* spec, void* scratch,
                 float* loss_out, float* dlogits, int ldd, float grad_scale, uwm_stream stream) {
  if (loss_ext_check("uwm_loss_ext", logits, ld, target, tdt, npix, spec, scratch)) return 1;
  if (!loss_out) return fail("uwm_loss_ext: bad argument");
  if (dlogits && ldd < 1) return fail("uwm_loss_ext: bad dlogits stride");
  LCHK(launch_loss_ext(logits, ld, target, tdt, (size_t)npix, *spec, (double*)scratch, loss_out, dlogits, ldd, grad_scale,
                       (hipStream_t)stream));
  return 0;
}
int uwm_loss_ext_sums(const float* logits, int ld, const void* target, int tdt, long long npix, const uwm_loss_spec* spec,
                      void* scratch, uwm_stream stream) {
  if (loss_ext_check("uwm_loss_ext_sums", logits, ld, target, tdt, npix, spec, scratch)) return 1;
  LCHK(launch_loss_ext_sums(logits, ld, target, tdt, (size_t)npix, *spec, (double*)scratch, (hipStream_t)stream));
  return 0;
}
int uwm_loss_ext_apply(const float* logits, int ld, const void* target, int tdt, long long npix, long long npix_total,
                       const uwm_loss_spec* spec, const void* scratch, float* loss_out, float* dlogits, int ldd, float grad_scale,
                       uwm_stream stream) {
  if (loss_ext_check("uwm_loss_ext_apply", logits, ld, target, tdt, npix, spec, scratch)) return 1;
  if (!loss_out || npix_total < npix) return fail("uwm_loss_ext_apply: bad argument");
  if (dlogits && ldd < 1) return fail("uwm_loss_ext_apply: bad dlogits stride");
  LCHK(launch_loss_ext_apply(logits, ld, target, tdt, (size_t)npix, (double)npix_total, *spec, (const double*)scratch, loss_out,
                             dlogits, ldd, grad_scale, (hipStream_t)stream));
  return 0;
}
int uwm_stats(const float* logits, int ld, const void* target, int tdt, int N, long long hw, float thr, int sig,
              long long* out, uwm_stream stream) {
  if (!logits || !target || !out || N < 1 || hw < 1) return fail("uwm_stats: bad argument");
  if (tdt < 0 || tdt > 3) return fail("uwm_stats: unsupported target dtype %d", tdt);
  LCHK(launch_stats(logits, ld, target, tdt, N, (size_t)hw, thr, sig, out, (hipStream_t)stream));
  return 0;
}
int uwm_threshold(const float* logits, int ld, long long npix, float thr, int sig, uint8_t* mask, uwm_stream stream) {
  if (!logits || !mask || npix < 1) return fail("uwm_threshold: bad argument");
  LCHK(launch_threshold(logits, ld, (size_t)npix, thr, sig, mask, (hipStream_t)stream));
  return 0;
}
int uwm_adam(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float wd,
             long long step, float gscale, uwm_stream stream) {
  if (!p || !g || !m || !v || n < 1 || step < 1) return fail("uwm_adam: bad argument");
  const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
  LCHK(launch_adam(p, g, m, v, (size_t)n, lr, b1, b2, eps, wd, bc1, bc2, gscale, (hipStream_t)stream));
  return 0;
}
int uwm_adam_clip(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float wd,
                  long long step, float gscale, float max_norm, void* scratch, uwm_stream stream) {
  if (!p || !g || !m || !v || !scratch || n < 1 || step < 1 || max_norm <= 0.f) return fail("uwm_adam_clip: bad argument");
  const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
  LCHK(launch_sumsq(g, (size_t)n, (double*)scratch, (hipStream_t)stream));
  LCHK(launch_adam(p, g, m, v, (size_t)n, lr, b1, b2, eps, wd, bc1, bc2, gscale, (hipStream_t)stream, (const double*)scratch, max_norm));
  return 0;
}
int uwm_adam_graph(float* p, const float* g, float* m, float* v, long long n, float* hyper, void* clip_scratch, uwm_stream stream) {
  if (!p || !g || !m || !v || !hyper || n < 1) return fail("uwm_adam_graph: bad argument");
  if (clip_scratch) LCHK(launch_sumsq(g, (size_t)n, (double*)clip_scratch, (hipStream_t)stream));
  LCHK(launch_adam_graph(p, g, m, v, (size_t)n, hyper, (const double*)clip_scratch, (hipStream_t)stream));
  return 0;
}
int uwm_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float wd,
              long long step, float gscale, uwm_stream stream) {
  if (!p || !g || !m || !v || n < 1 || step < 1) return fail("uwm_adamw: bad argument");
  const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
  LCHK(launch_adam(p, g, m, v, (size_t)n, lr, b1, b2, eps, wd, bc1, bc2, gscale, (hipStream_t)stream, nullptr, 0.f, true));
  return 0;
}
int uwm_adamw_clip(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float wd,
                   long long step, float gscale, float max_norm, void* scratch, uwm_stream stream) {
  if (!p || !g || !m || !v || !scratch || n < 1 || step < 1 || max_norm <= 0.f) return fail("uwm_adamw_clip: bad argument");
  const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
  LCHK(launch_sumsq(g, (size_t)n, (double*)scratch, (hipStream_t)stream));
  LCHK(launch_adam(p, g, m, v, (size_t)n, lr, b1, b2, eps, wd, bc1, bc2, gscale, (hipStream_t)stream, (const double*)scratch, max_norm, true));
  return 0;
}
int uwm_adamw_graph(float* p, const float* g, float* m, float* v, long long n, float* hyper, void* clip_scratch, uwm_stream stream) {
  if (!p || !g || !m || !v || !hyper || n < 1) return fail("uwm_adamw_graph: bad argument");
  if (clip_scratch) LCHK(launch_sumsq(g, (size_t)n, (double*)clip_scratch, (hipStream_t)stream));
  LCHK(launch_adam_graph(p, g, m, v, (size_t)n, hyper, (const double*)clip_scratch, (hipStream_t)stream, true));
  return 0;
}
int uwm_sgd(float* p, const float* g, float* buf, long long n, float lr, float momentum, float wd, long long step, float gscale,
            float max_norm, void* scratch, uwm_stream stream) {
  if (!p || !g || !buf || n < 1 || step < 1 || (max_norm > 0.f && !scratch)) return fail("uwm_sgd: bad argument");
  if (max_norm > 0.f) LCHK(launch_sumsq(g, (size_t)n, (double*)scratch, (hipStream_t)stream));
  LCHK(launch_sgd(p, g, buf, (size_t)n, lr, momentum, wd, step == 1, gscale, (hipStream_t)stream,
                  max_norm > 0.f ? (const double*)scratch : nullptr, max_norm));
  return 0;
}
int uwm_resize_threshold(const float* logits, int ld, int N, int h, int w, int H, int W, float threshold, int apply_sigmoid,
                         uint8_t* mask, float* resized, uwm_stream stream) {
  if (!logits || (!mask && !resized) || N < 1 || h < 1 || w < 1 || H < 1 || W < 1 || ld < 1) return fail("uwm_resize_threshold: bad argument");
  LCHK(launch_resize_threshold(logits, ld, N, h, w, H, W, threshold, apply_sigmoid, mask, resized, (hipStream_t)stream));
  return 0;
}
// ---- mask post-processing (mask_post.hip): every argument is checked here, before any launch
static int mask_shape_check(const char* fn, int N, int H, int W, const void* ws, size_t ws_bytes) {
  if (N < 1 || H < 1 || W < 1) return fail("%s: N, H, W must be >= 1 (got %d, %d, %d)", fn, N, H, W);
  if (N > 65535) return fail("%s: at most 65535 masks per call (got %d)", fn, N);
  if ((long long)H * W >= 2147483647ll) return fail("%s: H*W must be below 2^31 - 1 (got %d x %d)", fn, H, W);
  if (!ws) return fail("%s: null workspace", fn);
  if ((uintptr_t)ws & 15) return fail("%s: workspace must be 16-byte aligned", fn);
  const size_t need = mask_workspace_bytes(N, H, W);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  return 0;
}
int uwm_mask_element(int shape, int kw, int kh, uint8_t* out) {
  if (!out) return fail("uwm_mask_element: null argument");
  if (shape != UWM_MORPH_RECT && shape != UWM_MORPH_ELLIPSE) return fail("uwm_mask_element: unknown shape %d (UWM_MORPH_RECT = 0 | UWM_MORPH_ELLIPSE = 2)", shape);
  if (kw < 1 || kh < 1 || kw > 15 || kh > 15) return fail("uwm_mask_element: element size %d x %d outside 1..15", kw, kh);
  if (mask_element(shape, kw, kh, out)) return fail("uwm_mask_element: bad argument");
  return 0;
}
size_t uwm_mask_workspace_bytes(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1 || (long long)H * W >= 2147483647ll) { fail("uwm_mask_workspace_bytes: bad shape %d x %d x %d", N, H, W); return 0; }
  return mask_workspace_bytes(N, H, W);
}
int uwm_optimize_mask(const uint8_t* in, uint8_t* out, int N, int H, int W, int mask_type, long long* summary, void* ws,
                      size_t ws_bytes, uwm_stream stream) {
  if (!in || !out) return fail("uwm_optimize_mask: null argument");
  if (mask_type != UWM_MASK_WATERMARK && mask_type != UWM_MASK_TEXT && mask_type != UWM_MASK_MIXED)
    return fail("uwm_optimize_mask: unknown mask type %d (UWM_MASK_WATERMARK = 0 | UWM_MASK_TEXT = 1 | UWM_MASK_MIXED = 2)", mask_type);
  if ((uintptr_t)summary & 7) return fail("uwm_optimize_mask: summary must be 8-byte aligned");
  if (mask_shape_check("uwm_optimize_mask", N, H, W, ws, ws_bytes)) return 1;
  LCHK(launch_optimize_mask(in, out, N, H, W, mask_type, summary, ws, (hipStream_t)stream));
  return 0;
}
static int mask_ragged_caps_check(const char* fn, int N, size_t mask_bytes, long long rows) {
  if (N < 1 || mask_bytes < 1 || rows < 1) return fail("%s: N, mask_bytes and rows must be >= 1 (got %d, %zu, %lld)", fn, N, mask_bytes, rows);
  if (N > 65535) return fail("%s: N too large: at most 65535 masks per call (got %d)", fn, N);
  if (mask_bytes > ((size_t)1 << 40) || rows > (1ll << 40)) return fail("%s: mask_bytes and rows too large: at most 2^40 (got %zu, %lld)", fn, mask_bytes, rows);
  return 0;
}
size_t uwm_mask_ragged_workspace_bytes(int N, size_t mask_bytes, long long rows) {
  if (mask_ragged_caps_check("uwm_mask_ragged_workspace_bytes", N, mask_bytes, rows)) return 0;
  return mask_ragged_workspace_bytes(N, mask_bytes, rows);
}
int uwm_optimize_masks_ragged(const uint8_t* in, uint8_t* out, size_t mask_bytes, const uwm_image_desc* descs, int N, int mask_type,
                              long long max_pixels, long long rows, long long* stats, void* ws, size_t ws_bytes, uwm_stream stream) {
  const char* fn = "uwm_optimize_masks_ragged";
  if (!in || !out || !descs || !ws) return fail("%s: null argument", fn);
  if (mask_type != UWM_MASK_WATERMARK && mask_type != UWM_MASK_TEXT && mask_type != UWM_MASK_MIXED && mask_type != UWM_MASK_NONE)
    return fail("%s: unknown mask type %d (UWM_MASK_WATERMARK = 0 | UWM_MASK_TEXT = 1 | UWM_MASK_MIXED = 2 | UWM_MASK_NONE = 3)", fn, mask_type);
  if (mask_ragged_caps_check(fn, N, mask_bytes, rows)) return 1;
  if (max_pixels < 1) return fail("%s: max_pixels must be >= 1 (got %lld)", fn, max_pixels);
  if (max_pixels >= 2147483647ll) return fail("%s: max_pixels too large: it must be below 2^31 - 1 (got %lld)", fn, max_pixels);
  if (((uintptr_t)descs | (uintptr_t)stats | (uintptr_t)ws) & 7) return fail("%s: descriptors, stats and the workspace must be 8-byte aligned", fn);
  const size_t need = mask_ragged_workspace_bytes(N, mask_bytes, rows);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_optimize_masks_ragged(in, out, mask_bytes, (const ImageDesc*)descs, N, mask_type, max_pixels, rows, stats, ws, (hipStream_t)stream));
  return 0;
}
// ---- mask scoring (mask_score.hip): every argument is checked here, before any launch
size_t uwm_score_masks_workspace_bytes(int N, size_t mask_bytes, long long rows) {
  if (mask_ragged_caps_check("uwm_score_masks_workspace_bytes", N, mask_bytes, rows)) return 0;
  return score_masks_workspace_bytes(N, mask_bytes, rows);
}
int uwm_score_masks_ragged(const uint8_t* pred, const uint8_t* truth, size_t mask_bytes, const uwm_image_desc* descs, const int* radius, int N,
                           long long max_pixels, long long rows, long long* counts, void* ws, size_t ws_bytes, uwm_stream stream) {
  const char* fn = "uwm_score_masks_ragged";
  if (!pred || !truth || !descs || !radius || !counts || !ws) return fail("%s: null argument", fn);
  if (mask_ragged_caps_check(fn, N, mask_bytes, rows)) return 1;
  if (max_pixels < 1) return fail("%s: max_pixels must be >= 1 (got %lld)", fn, max_pixels);
  if (max_pixels >= 2147483647ll) return fail("%s: max_pixels too large: it must be below 2^31 - 1 (got %lld)", fn, max_pixels);
  if (((uintptr_t)descs | (uintptr_t)counts | (uintptr_t)ws) & 7) return fail("%s: descriptors, counts and the workspace must be 8-byte aligned", fn);
  if ((uintptr_t)radius & 3) return fail("%s: radius must be 4-byte aligned", fn);
  const size_t need = score_masks_workspace_bytes(N, mask_bytes, rows);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_score_masks_ragged(pred, truth, mask_bytes, (const ImageDesc*)descs, radius, N, max_pixels, rows, counts, ws, (hipStream_t)stream));
  return 0;
}
// ---- distance transforms and surface distances (mask_dist.hip): every argument is checked here, before any launch
static int dist_args_check(const char* fn, int N, size_t mask_bytes, long long max_pixels, long long rows) {
  if (mask_ragged_caps_check(fn, N, mask_bytes, rows)) return 1;
  if (max_pixels < 1) return fail("%s: max_pixels must be >= 1 (got %lld)", fn, max_pixels);
  if (max_pixels >= 2147483647ll) return fail("%s: max_pixels too large: it must be below 2^31 - 1 (got %lld)", fn, max_pixels);
  return 0;
}
size_t uwm_edt_workspace_bytes(int N, size_t mask_bytes, long long rows) {
  if (mask_ragged_caps_check("uwm_edt_workspace_bytes", N, mask_bytes, rows)) return 0;
  return edt_workspace_bytes(N, mask_bytes, rows);
}
int uwm_edt_ragged(const uint8_t* masks, size_t mask_bytes, const uwm_image_desc* descs, int N, long long max_pixels, long long rows, int* d2,
                   void* ws, size_t ws_bytes, uwm_stream stream) {
  const char* fn = "uwm_edt_ragged";
  if (!masks || !descs || !d2 || !ws) return fail("%s: null argument", fn);
  if (dist_args_check(fn, N, mask_bytes, max_pixels, rows)) return 1;
  if (((uintptr_t)descs | (uintptr_t)ws) & 7) return fail("%s: descriptors and the workspace must be 8-byte aligned", fn);
  if ((uintptr_t)d2 & 3) return fail("%s: d2 must be 4-byte aligned", fn);
  const size_t need = edt_workspace_bytes(N, mask_bytes, rows);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_edt_ragged(masks, mask_bytes, (const ImageDesc*)descs, N, max_pixels, rows, d2, ws, (hipStream_t)stream));
  return 0;
}
size_t uwm_surface_distances_workspace_bytes(int N, size_t mask_bytes, long long rows) {
  if (mask_ragged_caps_check("uwm_surface_distances_workspace_bytes", N, mask_bytes, rows)) return 0;
  return surface_distances_workspace_bytes(N, mask_bytes, rows);
}
int uwm_surface_distances_ragged(const uint8_t* pred, const uint8_t* truth, size_t mask_bytes, const uwm_image_desc* descs, int N,
                                 long long max_pixels, long long rows, long long* records, double* sums, void* ws, size_t ws_bytes,
                                 uwm_stream stream) {
  const char* fn = "uwm_surface_distances_ragged";
  if (!pred || !truth || !descs || !records || !sums || !ws) return fail("%s: null argument", fn);
  if (dist_args_check(fn, N, mask_bytes, max_pixels, rows)) return 1;
  if (((uintptr_t)descs | (uintptr_t)records | (uintptr_t)sums | (uintptr_t)ws) & 7)
    return fail("%s: descriptors, records, sums and the workspace must be 8-byte aligned", fn);
  const size_t need = surface_distances_workspace_bytes(N, mask_bytes, rows);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_surface_distances_ragged(pred, truth, mask_bytes, (const ImageDesc*)descs, N, max_pixels, rows, records, sums, ws, (hipStream_t)stream));
  return 0;
}
// ---- mask enhancement (mask_enhance.hip): every argument is checked here, before any launch
static int enhance_caps_check(const char* fn, int N, size_t mask_bytes) {
  if (N < 1 || mask_bytes < 1) return fail("%s: N and mask_bytes must be >= 1 (got %d, %zu)", fn, N, mask_bytes);
  if (N > 65535) return fail("%s: N too large: at most 65535 masks per call (got %d)", fn, N);
  if (mask_bytes > ((size_t)1 << 40)) return fail("%s: mask_bytes too large: at most 2^40 (got %zu)", fn, mask_bytes);
  return 0;
}
size_t uwm_enhance_masks_workspace_bytes(int N, size_t mask_bytes) {
  if (enhance_caps_check("uwm_enhance_masks_workspace_bytes", N, mask_bytes)) return 0;
  return enhance_workspace_bytes(N, mask_bytes);
}
int uwm_enhance_gauss_taps(int blur_kernel, float* out) {
  if (!out) { fail("uwm_enhance_gauss_taps: null argument"); return 0; }
  if (blur_kernel < 0 || blur_kernel > 63) { fail("uwm_enhance_gauss_taps: blur_kernel %d outside 0..63", blur_kernel); return 0; }
  return enhance_gauss_taps(blur_kernel, out);
}
int uwm_enhance_masks_ragged(const uint8_t* in, uint8_t* out, size_t mask_bytes, const uwm_image_desc* descs, int N, int expand_pixels,
                             int blur_kernel, int smooth_iterations, long long max_pixels, long long* stats, void* ws, size_t ws_bytes,
                             uwm_stream stream) {
  const char* fn = "uwm_enhance_masks_ragged";
  if (!in || !out || !descs || !ws) return fail("%s: null argument", fn);
  if (enhance_caps_check(fn, N, mask_bytes)) return 1;
  if (expand_pixels < 0 || expand_pixels > 31) return fail("%s: expand_pixels %d outside 0..31", fn, expand_pixels);
  if (blur_kernel < 0 || blur_kernel > 63) return fail("%s: blur_kernel %d outside 0..63", fn, blur_kernel);
  if (smooth_iterations < 0 || smooth_iterations > 8) return fail("%s: smooth_iterations %d outside 0..8", fn, smooth_iterations);
  if (max_pixels < 1) return fail("%s: max_pixels must be >= 1 (got %lld)", fn, max_pixels);
  if (max_pixels >= 2147483647ll) return fail("%s: max_pixels too large: it must be below 2^31 - 1 (got %lld)", fn, max_pixels);
  if (((uintptr_t)descs | (uintptr_t)stats | (uintptr_t)ws) & 7) return fail("%s: descriptors, stats and the workspace must be 8-byte aligned", fn);
  const size_t need = enhance_workspace_bytes(N, mask_bytes);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_enhance_masks_ragged(in, out, mask_bytes, (const ImageDesc*)descs, N, expand_pixels, blur_kernel, smooth_iterations, max_pixels,
                                   stats, ws, (hipStream_t)stream));
  return 0;
}
// ---- text-feature enhancement (text_enhance.hip): every argument is checked here, before any launch
static int text_enhance_caps_check(const char* fn, long long total_pixels, int N) {
  if (N < 1 || N > 65535) return fail("%s: N must be 1 .. 65535 (got %d)", fn, N);
  if (total_pixels < 1 || total_pixels > (1ll << 40)) return fail("%s: total_pixels must be 1 .. 2^40 (got %lld)", fn, total_pixels);
  return 0;
}
size_t uwm_text_enhance_workspace_bytes(long long total_pixels, int N) {
  if (text_enhance_caps_check("uwm_text_enhance_workspace_bytes", total_pixels, N)) return 0;
  return text_enhance_workspace_bytes(total_pixels, N);
}
int uwm_text_enhance_ragged(const uint8_t* in, uint8_t* out, size_t bytes, const uwm_image_desc* descs, int N, int C, long long max_pixels,
                            long long total_pixels, uint8_t* edges, size_t edges_bytes, const uwm_image_desc* edge_descs, void* ws,
                            size_t ws_bytes, uwm_stream stream) {
  const char* fn = "uwm_text_enhance_ragged";
  if (!in || !out || !descs || !ws) return fail("%s: null argument", fn);
  if (C != 3) return fail("%s: C must be 3 (RGB images; got %d)", fn, C);
  if (bytes < 1 || bytes > ((size_t)1 << 42)) return fail("%s: bytes must be 1 .. 2^42 (got %zu)", fn, bytes);
  if (text_enhance_caps_check(fn, total_pixels, N)) return 1;
  if (max_pixels < 1 || max_pixels > (1ll << 30)) return fail("%s: max_pixels must be 1 .. 2^30 (got %lld)", fn, max_pixels);
  if ((uintptr_t)in < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)in + bytes)
    return fail("%s: out must not overlap in (the sharpening filter reads neighbours)", fn);
  if (edges) {
    if (!edge_descs) return fail("%s: edges needs edge_descs", fn);
    if (edges_bytes < 1 || edges_bytes > ((size_t)1 << 40)) return fail("%s: edges_bytes must be 1 .. 2^40 (got %zu)", fn, edges_bytes);
    if ((uintptr_t)edges < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)edges + edges_bytes)
      return fail("%s: edges must not overlap out", fn);
  }
  if (((uintptr_t)descs | (uintptr_t)edge_descs | (uintptr_t)ws) & 7) return fail("%s: descriptors and the workspace must be 8-byte aligned", fn);
  const size_t need = text_enhance_workspace_bytes(total_pixels, N);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_text_enhance_ragged(in, out, bytes, (const ImageDesc*)descs, N, max_pixels, total_pixels, edges, edges ? edges_bytes : 0,
                                  (const ImageDesc*)edge_descs, ws, (hipStream_t)stream));
  return 0;
}
// ---- membrane fill (inpaint.hip): every argument is checked here, before any launch
static int inpaint_caps_check(const char* fn, int N, size_t image_bytes, int C, int max_side) {
  if (N < 1 || N > 65535) return fail("%s: N must be 1 .. 65535 (got %d)", fn, N);
  if (C < 1 || C > 4) return fail("%s: C must be 1 .. 4 (got %d)", fn, C);
  if (image_bytes < 1 || image_bytes > ((size_t)1 << 40)) return fail("%s: image_bytes must be 1 .. 2^40 (got %zu)", fn, image_bytes);
  if (max_side < 1 || max_side > 32768) return fail("%s: max_side must be 1 .. 32768 (got %d)", fn, max_side);
  return 0;
}
size_t uwm_inpaint_workspace_bytes(int N, size_t image_bytes, int C, int max_side) {
  if (inpaint_caps_check("uwm_inpaint_workspace_bytes", N, image_bytes, C, max_side)) return 0;
  return inpaint_workspace_bytes(N, image_bytes, C, max_side);
}
int uwm_inpaint_launch_count(int cycles, int max_side) {
  if (cycles < 0 || cycles > 32 || max_side < 1 || max_side > 32768) { fail("uwm_inpaint_launch_count: cycles 0 .. 32, max_side 1 .. 32768"); return 0; }
  return inpaint_launch_count(cycles, max_side);
}
int uwm_inpaint_ragged(const uint8_t* images, uint8_t* out, size_t image_bytes, const uwm_image_desc* img_descs, const uint8_t* masks,
                       size_t mask_bytes, const uwm_image_desc* mask_descs, int N, int C, int cycles, long long max_pixels, long long rows,
                       int max_side, long long* stats, void* ws, size_t ws_bytes, uwm_stream stream) {
  const char* fn = "uwm_inpaint_ragged";
  if (!images || !out || !img_descs || !masks || !mask_descs || !ws) return fail("%s: null argument", fn);
  if (inpaint_caps_check(fn, N, image_bytes, C, max_side)) return 1;
  if (mask_bytes < 1 || mask_bytes > ((size_t)1 << 40)) return fail("%s: mask_bytes must be 1 .. 2^40 (got %zu)", fn, mask_bytes);
  if (cycles < 0 || cycles > 32) return fail("%s: cycles %d outside 0..32", fn, cycles);
  if (max_pixels < 1 || max_pixels > (1ll << 30)) return fail("%s: max_pixels must be 1 .. 2^30 (got %lld)", fn, max_pixels);
  if (rows < 1 || rows > (1ll << 40)) return fail("%s: rows must be 1 .. 2^40 (got %lld)", fn, rows);
  if (out != images && (uintptr_t)images < (uintptr_t)out + image_bytes && (uintptr_t)out < (uintptr_t)images + image_bytes)
    return fail("%s: out must be images or must not overlap it", fn);
  if ((uintptr_t)masks < (uintptr_t)out + image_bytes && (uintptr_t)out < (uintptr_t)masks + mask_bytes)
    return fail("%s: out must not overlap masks", fn);
  if (((uintptr_t)img_descs | (uintptr_t)mask_descs | (uintptr_t)stats | (uintptr_t)ws) & 7)
    return fail("%s: descriptors, stats and the workspace must be 8-byte aligned", fn);
  const size_t need = inpaint_workspace_bytes(N, image_bytes, C, max_side);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_inpaint_ragged(images, out, image_bytes, (const ImageDesc*)img_descs, masks, mask_bytes, (const ImageDesc*)mask_descs, N, C, cycles,
                             max_pixels, rows, max_side, stats, ws, (hipStream_t)stream));
  return 0;
}
int uwm_op_morph(const uint8_t* in, uint8_t* out, int N, int H, int W, int dilate, int shape, int kw, int kh, int iterations,
                 void* ws, size_t ws_bytes, uwm_stream stream) {
  if (!in || !out) return fail("uwm_op_morph: null argument");
  if (shape != UWM_MORPH_RECT && shape != UWM_MORPH_ELLIPSE) return fail("uwm_op_morph: unknown shape %d (UWM_MORPH_RECT = 0 | UWM_MORPH_ELLIPSE = 2)", shape);
  if (kw < 1 || kh < 1 || kw > 15 || kh > 15) return fail("uwm_op_morph: element size %d x %d outside 1..15", kw, kh);
  if (iterations < 1) return fail("uwm_op_morph: iterations must be >= 1 (got %d)", iterations);
  if (mask_shape_check("uwm_op_morph", N, H, W, ws, ws_bytes)) return 1;
  LCHK(launch_mask_morph(in, out, N, H, W, dilate, shape, kw, kh, iterations, ws, (hipStream_t)stream));
  return 0;
}
int uwm_op_components(const uint8_t* in, int32_t* labels, int32_t* areas, int N, int H, int W, void* ws, size_t ws_bytes,
                      uwm_stream stream) {
  if (!in || !labels || !areas) return fail("uwm_op_components: null argument");
  if (((uintptr_t)labels | (uintptr_t)areas) & 3) return fail("uwm_op_components: labels and areas must be 4-byte aligned");
  if (mask_shape_check("uwm_op_components", N, H, W, ws, ws_bytes)) return 1;
  LCHK(launch_mask_components(in, labels, areas, N, H, W, ws, (hipStream_t)stream));
  return 0;
}
int uwm_preprocess_u8(const uint8_t* images, int N, int H, int W, int C, const float* mean, const float* std, const int* flags,
                      float* out_nchw, uwm_stream stream) {
  if (!images || !mean || !std || !out_nchw || N < 1 || H < 1 || W < 1 || C < 1 || C > 4) return fail("uwm_preprocess_u8: bad argument");
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_preprocess_u8: std[%d] must be positive", c);
  LCHK(launch_preprocess_u8(images, N, H, W, C, mean, std, flags, out_nchw, (hipStream_t)stream));
  return 0;
}
int uwm_preprocess_mask_u8(const uint8_t* masks, int N, int H, int W, int threshold, const int* flags, uint8_t* out,
                           uwm_stream stream) {
  if (!masks || !out || N < 1 || H < 1 || W < 1) return fail("uwm_preprocess_mask_u8: bad argument");
  LCHK(launch_preprocess_mask(masks, N, H, W, threshold, flags, out, (hipStream_t)stream));
  return 0;
}
// ---- train-time augmentation (augment_u8.hip).  The descriptors are device memory: what can be checked without reading them is
// checked here, before any launch; the kernels clamp the rest (they ignore rot90 where H != W and HSV shifts where C != 3)
static_assert(sizeof(uwm_aug_desc) == sizeof(AugDesc) && sizeof(uwm_aug_desc) == 320 && offsetof(uwm_aug_desc, minv) == 16 &&
              offsetof(uwm_aug_desc, lut) == 64 && offsetof(AugDesc, minv) == 16 && offsetof(AugDesc, lut) == 64, "uwm_aug_desc layout");
int uwm_augment_u8(const uint8_t* images, const uint8_t* masks, const uwm_aug_desc* descs, int N, int H, int W, int C, const float* mean,
                   const float* std, int mask_threshold, float* out_nchw, uint8_t* out_masks, uint8_t* out_u8, uwm_stream stream) {
  if (!images || !descs || !mean || !std || !out_nchw) return fail("uwm_augment_u8: null argument");
  if ((masks == nullptr) != (out_masks == nullptr)) return fail("uwm_augment_u8: masks and out_masks go together (both or neither)");
  if (C < 1 || C > 4) return fail("uwm_augment_u8: C must be 1..4 (got %d)", C);
  if (N < 1 || H < 1 || W < 1) return fail("uwm_augment_u8: N, H and W must be >= 1 (got %d, %d, %d)", N, H, W);
  if ((long long)N * ((H + 3) / 4) > 2147483647ll) return fail("uwm_augment_u8: N * H too large for one launch (%d x %d)", N, H);
  if ((uintptr_t)descs & 7) return fail("uwm_augment_u8: descriptors must be 8-byte aligned");
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_augment_u8: std[%d] must be positive", c);
  LCHK(launch_augment_u8(images, (const AugDesc*)descs, N, H, W, C, mean, std, out_nchw, out_u8, (hipStream_t)stream));
  if (masks) LCHK(launch_augment_mask(masks, (const AugDesc*)descs, N, H, W, mask_threshold, out_masks, (hipStream_t)stream));
  return 0;
}
// ---- the enhanced recipe's stages behind uwm_augment_u8 (augment_ext_u8.hip): the same checks, plus the workspace
static_assert(sizeof(uwm_aug_ext_desc) == sizeof(AugExtDesc) && sizeof(uwm_aug_ext_desc) == 296 && offsetof(uwm_aug_ext_desc, blur_w) == 16 &&
              offsetof(uwm_aug_ext_desc, seed) == 32 && offsetof(uwm_aug_ext_desc, lut2) == 40 && offsetof(AugExtDesc, blur_w) == 16 &&
              offsetof(AugExtDesc, seed) == 32 && offsetof(AugExtDesc, lut2) == 40, "uwm_aug_ext_desc layout");
size_t uwm_augment_ext_workspace_bytes(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 1 || C > 4) { fail("uwm_augment_ext_workspace_bytes: bad shape %d x %d x %d x %d", N, H, W, C); return 0; }
  return aug_ext_workspace_bytes(N, H, W, C);
}
int uwm_augment_ext_u8(const uint8_t* images, const uint8_t* masks, const uwm_aug_desc* descs, const uwm_aug_ext_desc* ext, int N, int H, int W,
                       int C, const float* mean, const float* std, int mask_threshold, void* workspace, size_t workspace_bytes,
                       float* out_nchw, uint8_t* out_masks, uint8_t* out_u8, uwm_stream stream) {
  if (!images || !descs || !mean || !std || !out_nchw) return fail("uwm_augment_ext_u8: null argument");
  if ((masks == nullptr) != (out_masks == nullptr)) return fail("uwm_augment_ext_u8: masks and out_masks go together (both or neither)");
  if (C < 1 || C > 4) return fail("uwm_augment_ext_u8: C must be 1..4 (got %d)", C);
  if (N < 1 || H < 1 || W < 1) return fail("uwm_augment_ext_u8: N, H and W must be >= 1 (got %d, %d, %d)", N, H, W);
  if ((long long)N * ((H + 3) / 4) > 2147483647ll || (long long)N * 64 > 2147483647ll)
    return fail("uwm_augment_ext_u8: N * H too large for one launch (%d x %d)", N, H);
  if (((uintptr_t)descs & 7) || ((uintptr_t)ext & 7)) return fail("uwm_augment_ext_u8: descriptors must be 8-byte aligned");
  for (int c = 0; c < C; ++c) if (!(std[c] > 0.f)) return fail("uwm_augment_ext_u8: std[%d] must be positive", c);
  if (ext) {
    if (!workspace) return fail("uwm_augment_ext_u8: null workspace");
    if ((uintptr_t)workspace & 15) return fail("uwm_augment_ext_u8: workspace must be 16-byte aligned");
    const size_t need = aug_ext_workspace_bytes(N, H, W, C);
    if (workspace_bytes < need) return fail("uwm_augment_ext_u8: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
  }
  const hipError_t e = launch_augment_ext(images, masks, (const AugDesc*)descs, (const AugExtDesc*)ext, N, H, W, C, mean, std, mask_threshold,
                                          workspace, workspace_bytes, out_nchw, out_masks, out_u8, (hipStream_t)stream);
  if (e == hipErrorStreamCaptureUnsupported)
    return fail("uwm_augment_ext_u8: the first call on a device uploads the tables and cannot be captured; call it once before capturing");
  LCHK(e);
  return 0;
}
int uwm_aug_lab_tables(int which, const void** data, int* count, int* elem_bytes) {
  if (!data || !count || !elem_bytes) return fail("uwm_aug_lab_tables: null argument");
  if (!aug_ext_host_table(which, data, count, elem_bytes)) return fail("uwm_aug_lab_tables: which must be 0..4 (got %d)", which);
  return 0;
}
// ---- ImageCompression of the transparent_watermark recipe (jpeg_u8.hip): every refusal comes before any launch
size_t uwm_jpeg_workspace_bytes(int N, int H, int W) {
  const size_t need = jpeg_workspace_bytes(N, H, W);
  if (!need) fail("uwm_jpeg_workspace_bytes: bad shape %d x %d x %d (N, H, W >= 1; H and W multiples of 16)", N, H, W);
  return need;
}
int uwm_jpeg_u8(const uint8_t* images, const int* quality, int N, int H, int W, const float* mean, const float* std, void* workspace,
                size_t workspace_bytes, float* out_nchw, uint8_t* out_u8, uwm_stream stream) {
  if (!images || !quality || !mean || !std) return fail("uwm_jpeg_u8: null argument");
  if (!out_nchw && !out_u8) return fail("uwm_jpeg_u8: out_nchw and out_u8 are both null");
  if (N < 1 || H < 1 || W < 1) return fail("uwm_jpeg_u8: N, H and W must be >= 1 (got %d, %d, %d)", N, H, W);
  if ((H & 15) || (W & 15)) return fail("uwm_jpeg_u8: H and W must be multiples of 16 (got %d, %d)", H, W);
  if ((long long)N * H * (W / 4) / 256 >= 2147483647ll) return fail("uwm_jpeg_u8: N * H * W too large for one launch (%d x %d x %d)", N, H, W);
  if ((uintptr_t)quality & 3) return fail("uwm_jpeg_u8: quality must be 4-byte aligned");
  if (((uintptr_t)images & 3) || ((uintptr_t)out_u8 & 3)) return fail("uwm_jpeg_u8: images and out_u8 must be 4-byte aligned");
  if ((uintptr_t)out_nchw & 15) return fail("uwm_jpeg_u8: out_nchw must be 16-byte aligned");
  for (int c = 0; c < 3; ++c) if (!(std[c] > 0.f)) return fail("uwm_jpeg_u8: std[%d] must be positive", c);
  if (!workspace) return fail("uwm_jpeg_u8: null workspace");
  if ((uintptr_t)workspace & 15) return fail("uwm_jpeg_u8: workspace must be 16-byte aligned");
  const size_t need = jpeg_workspace_bytes(N, H, W);
  if (workspace_bytes < need) return fail("uwm_jpeg_u8: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
  LCHK(launch_jpeg_u8(images, quality, N, H, W, mean, std, workspace, workspace_bytes, out_nchw, out_u8, (hipStream_t)stream));
  return 0;
}
// ---- the JPEG save of the synthesis chain (jpeg_ragged_u8.hip): every refusal comes before any launch
static int jpeg_ragged_caps_check(const char* fn, int N, size_t bytes) {
  if (N < 1 || N > 65535) return fail("%s: N must be 1 .. 65535 (got %d)", fn, N);
  if (bytes < 1 || bytes > ((size_t)1 << 42)) return fail("%s: bytes must be 1 .. 2^42 (got %zu)", fn, bytes);
  return 0;
}
size_t uwm_jpeg_ragged_workspace_bytes(int N, size_t bytes) {
  if (jpeg_ragged_caps_check("uwm_jpeg_ragged_workspace_bytes", N, bytes)) return 0;
  return bytes;                                                              // image i's planes lie at the image's own offset
}
int uwm_jpeg_ragged_u8(const uint8_t* in, uint8_t* out, size_t bytes, const uwm_image_desc* descs, const int* quality, int N, int C,
                       long long max_pixels, void* workspace, size_t workspace_bytes, uwm_stream stream) {
  const char* fn = "uwm_jpeg_ragged_u8";
  if (!in || !out || !descs || !quality || !workspace) return fail("%s: null argument", fn);
  if (C != 3) return fail("%s: C must be 3 (RGB images; got %d)", fn, C);
  if (jpeg_ragged_caps_check(fn, N, bytes)) return 1;
  if (max_pixels < 1) return fail("%s: max_pixels must be >= 1 (got %lld)", fn, max_pixels);
  if (max_pixels >= 2147483647ll) return fail("%s: max_pixels too large: it must be below 2^31 - 1 (got %lld)", fn, max_pixels);
  if (in != out && (uintptr_t)in < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)in + bytes)
    return fail("%s: out must be in itself or not overlap it", fn);
  if (((uintptr_t)in | (uintptr_t)out) & 3) return fail("%s: in and out must be 4-byte aligned", fn);
  if ((uintptr_t)quality & 3) return fail("%s: quality must be 4-byte aligned", fn);
  if (((uintptr_t)descs | (uintptr_t)workspace) & 7) return fail("%s: descriptors and the workspace must be 8-byte aligned", fn);
  if (workspace_bytes < bytes) return fail("%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes, bytes);
  if ((uintptr_t)workspace < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)workspace + bytes)
    return fail("%s: the workspace must not overlap out", fn);
  if ((uintptr_t)workspace < (uintptr_t)in + bytes && (uintptr_t)in < (uintptr_t)workspace + bytes)
    return fail("%s: the workspace must not overlap in", fn);
  LCHK(launch_jpeg_ragged_u8(in, out, bytes, (const ImageDesc*)descs, quality, N, max_pixels, workspace, workspace_bytes, (hipStream_t)stream));
  return 0;
}
int uwm_scale(float* p, long long n, float s, uwm_stream stream) {
  if (!p || n < 1) return fail("uwm_scale: bad argument");
  LCHK(launch_scale(p, (size_t)n, s, (hipStream_t)stream));
  return 0;
}

// ---- run-time switch for the internal weight-gradient side stream (default on; UWM_SIDE_STREAM=0 disables it)
int uwm_set_side_stream(uwm_handle h, int on) {
  if (!h) return fail("uwm_set_side_stream: null handle");
  h->use_side = on != 0; return 0;
}

// ---- HIP-event profiler (bench.py's roofline leg)
int uwm_prof_enable(int on) { prof_enable(on != 0); return 0; }
int uwm_prof_collect(double* out, int max_classes) {
  if (!out || max_classes < kProfClasses) return fail("uwm_prof_collect: need room for %d classes (4 doubles each)", (int)kProfClasses);
  prof_collect(out); return kProfClasses;
}
const char* uwm_prof_class_name(int cls) { return prof_class_name(cls); }

// ---- workspace introspection (parity tests): float offset + element count of a planned buffer.
// keys: "y:<conv>", "g:<conv>" (<conv> = state_dict prefix, e.g. encoder.layer1.0.conv1),
//       "xn:<i>", "gx:<i>" (encoder block i), "pool", "g_pool", "x4", "dcat:<i>", "gskip:<i>"
int uwm_debug_lookup(uwm_handle h, const char* key, long long* off, long long* count) {
  if (!h || !key || !off || !count) return fail("uwm_debug_lookup: null argument");
  const Plan& p = h->plan;
  const std::string k(key);
  // the fixed region (shape-independent): "fixed" = all of it; "bnf:<bn>" = a BatchNorm's {scale, shift}; "wu:<conv>" / "wud:<conv>" /
  // "wd:<conv>" = a conv's forward bank slot / dgrad bank slot / dgrad repack (count 0 where the layer has none)
  if (k == "fixed") { *off = 0; *count = (long long)h->fixed_floats; return 0; }
  if (k.rfind("bnf:", 0) == 0) {
    for (auto& b : h->bns) if (b.name == k.substr(4)) { *off = (long long)(b.f_off + 2 * (size_t)b.C); *count = 2LL * b.C; return 0; }
    return fail("uwm_debug_lookup: unknown BatchNorm %s", k.c_str() + 4);
  }
  if (k.rfind("wu:", 0) == 0 || k.rfind("wud:", 0) == 0 || k.rfind("wd:", 0) == 0) {
    const std::string name = k.substr(k.find(':') + 1);
    for (auto& cv : h->convs) if (cv.name == name) {
      if (k[1] == 'd') { *off = (long long)cv.wd_off; *count = cv.dgrad ? (long long)cv.CinP * cv.KpadD : 0; }
      else if (k[2] == 'd') { *off = (long long)cv.wud_off; *count = cv.wud_off ? (long long)std::max(wino_weights_floats(cv.CinP, cv.CoutP), cv.f3_d() ? f16x3_bank_floats(cv.CinP, cv.CoutP) : 0) : 0; }
      else { *off = (long long)cv.wu_off; *count = (long long)cv.wu_floats; }
      return 0;
    }
    return fail("uwm_debug_lookup: unknown conv %s", name.c_str());
  }
  if (p.N == 0) return fail("uwm_debug_lookup: no plan yet");
  const int N = p.N, H = p.H, W = p.W;
  auto conv_geo = [&](int ci, long long* cnt) { *cnt = (long long)N * p.oh[ci] * p.ow[ci] * h->convs[ci].CoutP; };
  if (k.rfind("y:", 0) == 0 || k.rfind("g:", 0) == 0) {
    const std::string name = k.substr(2);
    for (size_t i = 0; i < h->convs.size(); ++i) if (h->convs[i].name == name) {
      if ((int)i == h->head) return fail("uwm_debug_lookup: head output is the caller's logits buffer");
      *off = (long long)(k[0] == 'y' ? p.y[i] : p.g[i]); conv_geo((int)i, count); return 0;
    }
    return fail("uwm_debug_lookup: unknown conv %s", name.c_str());
  }
  auto blk_geo = [&](size_t bi, long long* cnt) {
    if (!h->mb.empty()) { *cnt = bi < h->mb.size() ? (long long)N * p.mh[bi] * p.mw[bi] * h->mb[bi].Cout : 0; return; }
    int hh = H / 4, ww = W / 4; size_t b = 0;
    for (int s = 0; s < 4; ++s) for (auto& bl : h->stages[s]) {
      hh /= bl.stride; ww /= bl.stride;
      if (b == bi) { *cnt = (long long)N * hh * ww * bl.Cout; return; }
      ++b;
    }
    *cnt = 0;
  };
  if (k.rfind("xn:", 0) == 0 || k.rfind("gx:", 0) == 0) {
    const size_t bi = (size_t)atoi(k.c_str() + 3);
    if (bi >= p.xn.size()) return fail("uwm_debug_lookup: bad block index");
    *off = (long long)(k[0] == 'x' ? p.xn[bi] : p.gx[bi]); blk_geo(bi, count); return 0;
  }
  if (k == "stem_a") { *off = (long long)p.stem_a; *count = (long long)N * (H / 2) * (W / 2) * h->f1C; return 0; }
  if (k == "pool" || k == "g_pool") { *off = (long long)(k == "pool" ? p.pool : p.g_pool); *count = (long long)N * (H / 4) * (W / 4) * 64; return 0; }
  if (k == "x4") { *off = (long long)p.x4; *count = (long long)N * H * W * h->CinP; return 0; }
  if (k.rfind("dcat:", 0) == 0 || k.rfind("gskip:", 0) == 0) {
    const bool dc = k[0] == 'd';
    const size_t i = (size_t)atoi(k.c_str() + (dc ? 5 : 6));
    if (i >= h->dec.size() || p.dcat.empty()) return fail("uwm_debug_lookup: bad decoder index / eval plan");
    const int hh = (H / 32) << (i + 1), ww = (W / 32) << (i + 1);
    *off = (long long)(dc ? p.dcat[i] : p.gskip[i]);
    *count = (long long)N * hh * ww * (dc ? h->dec[i].C0 + h->dec[i].C1 : h->dec[i].C1);
    return 0;
  }
  return fail("uwm_debug_lookup: unknown key %s", key);
}

// ---- single-operator entry points
// Winograd weights for the op-level entry points (tests): transformed into a cached scratch buffer
static int op_wino_prepare(ConvArgs& a, int mirror, hipStream_t st, bool x3 = false) {
  static float* buf = nullptr; static size_t cap = 0;
  const size_t need = wino_weights_floats(a.wrows, a.Ctot);
  if (need > cap) {
    HIPCHK(hipDeviceSynchronize());
    if (buf) HIPCHK(hipFree(buf));
    HIPCHK(hipMalloc((void**)&buf, need * sizeof(float))); cap = need;
  }
  if (x3) {           // bf16x3 bank (forward layout only: the model derives dgrad banks from the forward weights itself)
    if (mirror || (a.Ctot & 15)) return fail("uwm_op_conv: cfg 400 (bf16x3 Winograd) takes forward weights with channels %% 16 == 0");
    WinoJobs jobs; jobs.n = 1;
    WinoJob& j = jobs.j[0];
    j.w = a.w; j.ut = buf; j.rows = a.wrows; j.chans = a.Ctot; j.Kpad = a.Kpad; j.mode = 0; j.src_rows = a.wrows; j.pad_ = 0;
    LCHK(launch_wino_weights_x3_multi(jobs, st));
    a.prec = 1;
  } else {
    LCHK(launch_wino_weights(a.w, a.wrows, a.Kpad, a.Ctot, mirror, buf, st));
  }
  a.wu = buf; a.wu_ncb = wino_ncb(a.wrows);
  return 0;
}
static int g_op_f3_nprod = 3;                     // ConvArgs::nprod of the op-level fp16x3 direct launches (uwm_op_conv cfg 600..607, uwm_op_dgrad_f16x3) and WgradArgs::nprod of uwm_op_wgrad force 6 / 7
int uwm_op_set_f16x3_products(int n) {            // tests: split products per tile of those launches (the model takes its count from the precision mode)
  if (n < 1 || n > 3) return fail("uwm_op_set_f16x3_products: n must be 1, 2 or 3, got %d", n);
  g_op_f3_nprod = n; return 0;
}
// fp16x3 bank for the op-level entry point (tests / timing): cfg 600
static int op_f16x3_prepare(ConvArgs& a, hipStream_t st, int variant = 0, bool reuse = false) {
  static float* buf = nullptr; static size_t cap = 0;
  static const float* last_w = nullptr; static int last_rows = 0, last_chans = 0, last_layout = -1;      // kernel timing (cfg + 1000): the bank of the previous call is reused when it matches
  if ((a.Ctot & 31) && !(a.Ctot == 16 && a.Cout <= 16)) return fail("uwm_op_conv: cfg 600 (fp16x3) needs channels %% 32 == 0 (or the 16 -> 16 single-chunk layer)");
  const size_t need = f16x3_bank_floats(a.wrows, a.Ctot);
  if (need > cap) {
    HIPCHK(hipDeviceSynchronize());
    if (buf) HIPCHK(hipFree(buf));
    HIPCHK(hipMalloc((void**)&buf, need * sizeof(float))); cap = need;
  }
  WinoJobs jobs; jobs.n = 1;
  WinoJob& j = jobs.j[0];
  // bank layout: 601-603 force a conv_f16x3.hip kernel (layout 0), 605 / 607 a conv_f16x3v2.hip one (layout 1), 600 = what the model would take
  const int layout = variant >= 4 ? 1 : (variant == 0 && f16x3v2_shape(a.Ho, a.Wo, a.wrows, a.Ctot) && a.wrows == a.Cout ? 1 : 0);
  j.w = a.w; j.ut = buf; j.rows = a.wrows; j.chans = a.Ctot; j.Kpad = a.Kpad; j.mode = 0; j.src_rows = a.wrows; j.pad_ = layout;
  a.wu = buf; a.wu_layout = layout; a.wu_ncb = layout == 1 ? f16x3v2_nf(a.wrows) : f16x3_nj(a.wrows); a.wu_rinv_off = (int)f16x3_rinv_off(a.wrows, a.Ctot); a.prec = 2;
  a.nprod = g_op_f3_nprod;
  if (conv_route(a, 600 + variant).k == kConvInvalid) return fail("uwm_op_conv: cfg %d: the coded fp16x3 kernel does not take this shape", 600 + variant);      // (before the bank launch: a rejected call launches nothing)
  if (!(reuse && last_w == a.w && last_rows == a.wrows && last_chans == a.Ctot && last_layout == layout)) LCHK(launch_f16x3_weights_multi(jobs, st));
  last_w = a.w; last_rows = a.wrows; last_chans = a.Ctot; last_layout = layout;
  return 0;
}
static bool op_wino_shape(const ConvArgs& a, int kh, int kw, int stride, int pad) {
  return kh == 3 && kw == 3 && stride == 1 && pad == 1 && (a.Ctot & 7) == 0 && (a.C0 & 7) == 0 && a.Ho >= 8 && a.Wo >= 16;
}
int uwm_set_join_stream(uwm_handle h, uwm_stream stream) {
  if (!h) return fail("uwm_set_join_stream: null handle");
  h->join_stream = (hipStream_t)stream; return 0;
}
int uwm_set_drop_connect(uwm_handle h, const float* rowscale) {
  if (!h) return fail("uwm_set_drop_connect: null handle");
  if (rowscale && h->mb.empty()) return fail("uwm_set_drop_connect: the encoder has no MBConv blocks");
  h->keep = rowscale; return 0;
}
int uwm_num_mbconv_blocks(uwm_handle h) { return h ? (int)h->mb.size() : 0; }
float uwm_mbconv_drop_rate(uwm_handle h, int block) {
  if (!h || block < 0 || block >= (int)h->mb.size()) return 0.f;
  return h->mb[block].skip ? h->mb[block].drop : 0.f;
}
int uwm_op_depthwise(int mode, const float* a, const float* b, int k, int stride, int pb, int N, int H, int W, int C, int Ho, int Wo,
                     const float* addend, float* out, float* scratch, uwm_stream stream) {
  if (!a || !b || !out || N < 1 || (C & 3) || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return fail("uwm_op_depthwise: bad argument");
  if (pb < 0 || pb >= k || Ho < 1 || Wo < 1 || (Ho - 1) * stride - pb >= H || (Wo - 1) * stride - pb >= W) return fail("uwm_op_depthwise: bad geometry");
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0) LCHK(launch_dw_fwd(a, b, k, stride, pb, N, H, W, C, Ho, Wo, out, st));
  else if (mode == 1) LCHK(launch_dw_dgrad(a, b, k, stride, pb, N, H, W, C, Ho, Wo, addend, out, st));
  else if (mode == 2) { if (!scratch) return fail("uwm_op_depthwise: wgrad needs scratch"); LCHK(launch_dw_wgrad(a, b, k, stride, pb, N, H, W, C, Ho, Wo, out, scratch, st)); }
  else return fail("uwm_op_depthwise: bad mode %d", mode);
  return 0;
}
long long uwm_op_depthwise_scratch_floats(int k, int N, int C, int Ho, int Wo) { return (long long)dw_wgrad_scratch_floats(k, N, C, Ho, Wo); }
// Single-operator entry points of the MBConv plumbing (mbconv.hip) and the depthwise BatchNorm statistics: tests and kernel
// timing.  Each checks its arguments on the host, zeroes what the model zeroes for the launcher, and calls the launcher the
// forward / backward calls.  (A C with no channel slice, pick_cw(C) == 0, is refused by the reducing launchers themselves
// before they launch; with C % 4 == 0 and C >= 4 there always is one.)
static bool op_nc_bad(int N, long long hw, int C) { return N < 1 || hw < 1 || C < 4 || (C & 3); }
int uwm_op_swish(const float* y, const float* scale, const float* shift, long long npix, int C, float* out, uwm_stream stream) {
  if (!y || !scale || !shift || !out || op_nc_bad(1, npix, C)) return fail("uwm_op_swish: bad argument");
  LCHK(launch_swish_fwd(y, scale, shift, C, out, (size_t)npix, (hipStream_t)stream));
  return 0;
}
long long uwm_op_se_scratch_floats(int N, int C) { return (N < 1 || C < 4 || (C & 3)) ? 0 : (long long)se_reduce_scratch_floats(N, C); }
int uwm_op_swish_pool(const float* y, const float* scale, const float* shift, int N, long long hw, int C, float* act_out,
                      float* pool, float* part, uwm_stream stream) {
  if (!y || !scale || !shift || !act_out || !pool || !part || op_nc_bad(N, hw, C) || N > 65535) return fail("uwm_op_swish_pool: bad argument");
  LCHK(launch_swish_pool(y, scale, shift, act_out, N, (size_t)hw, C, pool, part, (hipStream_t)stream));
  return 0;
}
int uwm_op_se_reduce(const float* a, const float* b, int N, long long hw, int C, float mult, float* out, float* part,
                     uwm_stream stream) {
  if (!a || !out || !part || op_nc_bad(N, hw, C) || N > 65535) return fail("uwm_op_se_reduce: bad argument");
  LCHK(launch_se_reduce_hw(a, b, N, (size_t)hw, C, mult, out, part, (hipStream_t)stream));
  return 0;
}
static bool op_fc_bad(int K1pad, int K2pad, int N, int C, int nsq) {
  return op_nc_bad(N, 1, C) || N > 65535 || nsq < 1 || nsq > 8192 || K1pad < C || K2pad < (int)rup(nsq, 4) || (K2pad & 3);
}
int uwm_op_se_fc(const float* pool, const float* w1, const float* b1, int K1pad, const float* w2, const float* b2, int K2pad,
                 int N, int C, int nsq, float* hpre, float* hid, float* s, uwm_stream stream) {
  if (!pool || !w1 || !b1 || !w2 || !b2 || !hpre || !hid || !s || op_fc_bad(K1pad, K2pad, N, C, nsq)) return fail("uwm_op_se_fc: bad argument");
  if ((uintptr_t)w2 & 15) return fail("uwm_op_se_fc: w2 must be 16-byte aligned");
  LCHK(launch_se_fc_fwd(pool, w1, b1, K1pad, w2, b2, K2pad, N, C, nsq, hpre, hid, s, (hipStream_t)stream));
  return 0;
}
int uwm_op_se_fc_backward(float* gs, const float* s, const float* hpre, const float* pool, const float* w1, int K1pad,
                          const float* w2, int K2pad, int N, int C, int nsq, float* gpool, float* acc1, float* gw1, float* gb1,
                          float* gw2, float* gb2, uwm_stream stream) {
  if (!gs || !s || !hpre || !pool || !w1 || !w2 || !gpool || !acc1 || !gw1 || !gb1 || !gw2 || !gb2 || op_fc_bad(K1pad, K2pad, N, C, nsq))
    return fail("uwm_op_se_fc_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(acc1, 0, (size_t)N * nsq * sizeof(float), st));
  LCHK(launch_se_fc_bwd(gs, s, hpre, pool, w1, K1pad, w2, K2pad, N, C, nsq, gpool, acc1, gw1, gb1, gw2, gb2, st));
  return 0;
}
int uwm_op_se_scale(const float* a, const float* s, int N, long long hw, int C, float* out, uwm_stream stream) {
  if (!a || !s || !out || op_nc_bad(N, hw, C)) return fail("uwm_op_se_scale: bad argument");
  LCHK(launch_se_scale(a, s, N, (size_t)hw, C, out, (hipStream_t)stream));
  return 0;
}
int uwm_op_mb_out(const float* y, const float* scale, const float* shift, const float* rowscale, const float* id, int N,
                  long long hw, int C, float* out, uwm_stream stream) {
  if (!y || !scale || !shift || !out || op_nc_bad(N, hw, C)) return fail("uwm_op_mb_out: bad argument");
  LCHK(launch_mb_out(y, scale, shift, rowscale, id, N, (size_t)hw, C, out, (hipStream_t)stream));
  return 0;
}
int uwm_op_rowscale(const float* g, const float* rowscale, int N, long long hw, int C, float* out, uwm_stream stream) {
  if (!g || !rowscale || !out || op_nc_bad(N, hw, C)) return fail("uwm_op_rowscale: bad argument");
  LCHK(launch_rowscale(g, rowscale, N, (size_t)hw, C, out, (hipStream_t)stream));
  return 0;
}
int uwm_op_bn_stats(const float* y, long long npix, int C, const float* gamma, const float* beta, float eps, float momentum,
                    int update_running, float* run_mean, float* run_var, double* sums2c, float* mean, float* rstd, float* scale,
                    float* shift, uwm_stream stream) {
  if (!y || !gamma || !beta || !sums2c || !mean || !rstd || !scale || !shift || op_nc_bad(1, npix, C) ||
      (update_running && (!run_mean || !run_var)))
    return fail("uwm_op_bn_stats: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(sums2c, 0, 2 * (size_t)C * sizeof(double), st));
  LCHK(launch_colstats(y, (size_t)npix, C, sums2c, sums2c + C, st));
  LCHK(launch_bn_finalize(sums2c, sums2c + C, gamma, beta, run_mean, run_var, mean, rstd, scale, shift, C, (double)npix, eps,
                          momentum, update_running != 0, st, 1, 2 * C));
  return 0;
}
int uwm_set_winograd(int on) { winograd_set_mode(on < 0 ? 0 : (on > 2 ? 1 : on)); return 0; }
int uwm_set_winograd_mode(uwm_handle h, int mode) {
  if (!h) return fail("uwm_set_winograd_mode: null handle");
  if (mode < 0 || mode > 2) return fail("uwm_set_winograd_mode: mode must be 0 (direct kernels), 1 (auto) or 2 (8-wave variant wherever allowed), got %d", mode);
  h->wino_mode = mode; h->plan.wino_mode = mode;       // the workspace layout does not depend on the mode
  return 0;
}
int uwm_get_winograd_mode(uwm_handle h) { return h ? h->wino_mode : -1; }
int uwm_set_precision(uwm_handle h, int mode) {
  if (!h) return fail("uwm_set_precision: null handle");
  if (mode < UWM_PREC_F32 || mode > UWM_PREC_F16X3_BWD2)
    return fail("uwm_set_precision: mode must be UWM_PREC_F32 (0), UWM_PREC_BF16X3 (1), UWM_PREC_BF16X3_ALL (2), UWM_PREC_F16X3 (3), UWM_PREC_F16X3_ALL (4), UWM_PREC_F16X1 (5) or UWM_PREC_F16X3_BWD2 (6), got %d", mode);
  h->prec = mode; h->plan.prec = mode;          // the workspace layout does not depend on the mode (the banks have one size)
  return 0;
}
int uwm_get_precision(uwm_handle h) { return h ? h->prec : -1; }
int uwm_set_precision_fill(uwm_handle h, int min_workgroups) {
  if (!h || min_workgroups < 0) return fail("uwm_set_precision_fill: bad argument");
  h->f3_min_wgs = min_workgroups; return 0;
}
int uwm_set_routing_batch(uwm_handle h, int batch) {
  if (!h || batch < 0 || batch > 255) return fail("uwm_set_routing_batch: batch must be 0 (= the real batch) .. 255");
  h->route_n = batch; return 0;
}
int uwm_routing_enable(uwm_handle h, int on) {
  if (!h) return fail("uwm_routing_enable: null handle");
  h->route_log_on = on != 0; if (!on) h->route_log.clear();
  return 0;
}
long long uwm_routing_dump(uwm_handle h, char* buf, long long cap, int clear) {
  if (!h) return -1;
  const long long need = (long long)h->route_log.size() + 1;
  if (buf && cap > 0) {
    const long long n = need <= cap ? need - 1 : cap - 1;
    memcpy(buf, h->route_log.data(), (size_t)n); buf[n] = 0;
  }
  if (clear) h->route_log.clear();
  return need;
}

// ---- data-parallel exchange on the C ABI (SURVEY.md 8b/8e): SUM all-reduce of the gradient arena ranges of backward
// stages [stage_begin, stage_end) over an RCCL communicator, one collective per stage (= bucket), enqueued on `stream`.
// RCCL is resolved at run time from the process (the library the caller's communicator came from), never linked.
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
static nccl_allreduce_fn g_allreduce = nullptr;
static int resolve_rccl() {
  if (g_allreduce) return 0;
  void* sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
  if (!sym) {
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (lib) sym = dlsym(lib, "ncclAllReduce");
  }
  if (!sym) return fail("uwm_allreduce_grads: ncclAllReduce not found (load RCCL in the host process first)");
  g_allreduce = (nccl_allreduce_fn)sym; return 0;
}
int uwm_allreduce_grads(uwm_handle h, void* comm, int sb, int se, uwm_stream stream) {
  if (!h || !comm) return fail("uwm_allreduce_grads: null argument");
  if (!h->grads) return fail("uwm_allreduce_grads: no gradient arena bound");
  if (sb < 0 || se > h->nstages || sb >= se) return fail("uwm_allreduce_grads: bad stage range [%d,%d)", sb, se);
  if (resolve_rccl()) return 1;
  DeviceGuard guard(h->device);
  for (int k = sb; k < se; ++k) {
    const long long b = h->stage_begin[k], e = h->stage_begin[k + 1];
    if (e <= b) continue;
    const int rc = g_allreduce(h->grads + b, h->grads + b, (size_t)(e - b), /*ncclFloat32*/ 7, /*ncclSum*/ 0, comm, (hipStream_t)stream);
    if (rc != 0) return fail("uwm_allreduce_grads: ncclAllReduce failed on bucket %d (ncclResult_t %d)", k, rc);
  }
  return 0;
}
float* uwm_grad_arena(uwm_handle h) { return h ? h->grads : nullptr; }
static Src to_src(const uwm_src* s) { return mk_src(s->ptr, s->C, s->H, s->W, s->scale, s->shift, s->relu, s->up); }

static int g_op_ig16 = 0;                          // 0 exact fp32 | 1 fp16x3, weight operand pre-split into a bank (what the model runs) | 2 fp16x3, split while staging
// the bank of a single-operator launch, built on the fly (the model builds its banks once per step): one job of the fp16x3 bank launch
static int op_ig_bank(const float* w, int rows, int Kpad, int slot, hipStream_t st, const float** bank) {
  static float* buf[2] = {nullptr, nullptr}; static size_t cap[2] = {0, 0};
  const size_t n = (size_t)rows * Kpad;
  if (n > cap[slot]) {
    if (buf[slot]) HIPCHK(hipFree(buf[slot]));     // (waits for the launches that still read it)
    buf[slot] = nullptr; cap[slot] = 0;
    HIPCHK(hipMalloc((void**)&buf[slot], n * sizeof(float)));
    cap[slot] = n;
  }
  WinoJobs jobs; memset(&jobs, 0, sizeof(jobs)); jobs.n = 1;
  jobs.j[0].w = w; jobs.j[0].ut = buf[slot]; jobs.j[0].rows = rows; jobs.j[0].Kpad = Kpad; jobs.j[0].mode = 3; jobs.j[0].src_rows = rows;
  LCHK(launch_f16x3_weights_multi(jobs, st));
  *bank = buf[slot];
  return 0;
}
int uwm_op_set_igemm_f16x3(int on) { g_op_ig16 = on == 2 ? 2 : (on != 0); return 0; }      // tests / kernel timing: the single-operator conv / dgrad entry points take the implicit GEMM's fp16x3 form (ConvArgs::ig16)
int uwm_op_conv(const uwm_src* s0, const uwm_src* s1, const float* w, int wrows, int Kpad, int kh, int kw, int stride,
                int pad, int N, int Cout, const float* bias, float* y, double* stats, int cfg, uwm_stream stream) {
  if (!s0 || !w || !y) return fail("uwm_op_conv: null argument");
  ConvArgs a; memset(&a, 0, sizeof(a));
  a.s0 = to_src(s0); a.C0 = a.s0.C;
  if (s1) { a.s1 = to_src(s1); a.Ctot = a.C0 + a.s1.C; } else { a.s1 = a.s0; a.Ctot = a.C0; }
  a.Hl = a.s0.H << a.s0.up; a.Wl = a.s0.W << a.s0.up;
  a.w = w; a.wrows = wrows; a.Kpad = Kpad; a.ntaps = kh * kw; a.kw = kw;
  a.N = N; a.Ho = (a.Hl + 2 * pad - kh) / stride + 1; a.Wo = (a.Wl + 2 * pad - kw) / stride + 1;
  a.Cout = Cout; a.M = N * a.Ho * a.Wo;
  a.smul = stride; a.rmul = 1; a.off = -pad; a.sdiv = 1;
  a.out = y; a.bias = bias;
  if (stats) { a.ssum = stats; a.ssq = stats + Cout; }
  a.dv_ctot = make_fastdiv(a.Ctot); a.dv_kw = make_fastdiv(a.kw);
  a.ig16 = g_op_ig16 != 0;
  if (g_op_ig16 == 1 && !(Kpad & 31) && cfg < 6 && conv_route(a, cfg).k == kConvIgemm && op_ig_bank(w, wrows, Kpad, 0, (hipStream_t)stream, &a.wbank)) return 1;
  if (cfg == 610) {                                     // the ResNet stem on conv_stem_f16x3.hip
    static float* sbuf = nullptr;
    if (!sbuf) HIPCHK(hipMalloc((void**)&sbuf, stem_f16x3_bank_floats() * sizeof(float)));
    if (kh != 7 || kw != 7 || a.Ctot != 4 || wrows != 64) return fail("uwm_op_conv: cfg 610 is the 7x7 stem (4 stored input channels, 64 outputs)");
    LCHK(launch_stem_f16x3_weights(w, Kpad, a.Ctot, sbuf, (hipStream_t)stream));
    a.wu = sbuf;
    LCHK(launch_conv_stem_f16x3(a, (hipStream_t)stream));
    return 0;
  }
  const bool reuse_bank = cfg >= 1600 && cfg <= 1607;      // 16xx = 6xx without re-packing the filter bank (kernel-only timing: the previous call must have been the same layer and layout)
  if (reuse_bank) cfg -= 1000;
  if (cfg == 604 || cfg == 606) return fail("uwm_op_conv: cfg %d names a removed conv_f16x3v2 form (607 is its kernel)", reuse_bank ? cfg + 1000 : cfg);
  if (cfg >= 600 && cfg <= 607) {                     // the codes: include/uwm.h
    if (!op_wino_shape(a, kh, kw, stride, pad)) return fail("uwm_op_conv: cfg 600 (fp16x3) needs 3x3 s1 p1, Ho >= 8, Wo >= 16");
    if (op_f16x3_prepare(a, (hipStream_t)stream, cfg - 600, reuse_bank)) return 1;
  } else if (((cfg >= 300 && cfg < 500) || (cfg < 0 && winograd_mode() != 0)) && op_wino_shape(a, kh, kw, stride, pad)) {
    if (op_wino_prepare(a, 0, (hipStream_t)stream, cfg == 400)) return 1;
  } else if (cfg >= 300 && cfg < 500) return fail("uwm_op_conv: cfg 300 (Winograd) needs 3x3 s1 p1, channels %% 8 == 0, Ho >= 8, Wo >= 16");
  LCHK(launch_conv(a, (hipStream_t)stream, cfg));
  return 0;
}
int uwm_op_dgrad(const float* dy, int N, int Ho, int Wo, int Cout, const float* wd, int Cin, int KpadD, int kh, int kw,
                 int stride, int pad, int H, int W, const float* addend, const float* mask, const float* mscale,
                 const float* mshift, float* dx, uwm_stream stream) {
  if (!dy || !wd || !dx) return fail("uwm_op_dgrad: null argument");
  ConvArgs a; memset(&a, 0, sizeof(a));
  a.s0 = mk_src(dy, Cout, Ho, Wo); a.s1 = a.s0; a.C0 = Cout; a.Ctot = Cout;
  a.w = wd; a.wrows = Cin; a.Kpad = KpadD; a.ntaps = kh * kw; a.kw = kw;
  a.N = N; a.Ho = H; a.Wo = W; a.Cout = Cin; a.M = N * H * W;
  a.Hl = Ho; a.Wl = Wo; a.smul = 1; a.rmul = -1; a.off = pad; a.sdiv = stride;
  a.out = dx; a.addend = addend; a.mask = mask; a.mscale = mscale; a.mshift = mshift;
  a.dv_ctot = make_fastdiv(a.Ctot); a.dv_kw = make_fastdiv(a.kw);
  if (g_op_ig16) {                                 // fp16x3 implicit GEMM: max|dy| through a one-off reduction (the model takes it from bn_bwd_apply)
    static float* xm = nullptr;
    if (!xm) HIPCHK(hipMalloc((void**)&xm, 32 * sizeof(float)));
    LCHK(launch_absmax32(dy, (size_t)N * Ho * Wo * Cout, xm, (hipStream_t)stream));
    a.ig16 = 1; a.xmax = xm;
  }
  if (winograd_mode() != 0 && op_wino_shape(a, kh, kw, stride, pad) && op_wino_prepare(a, 1, (hipStream_t)stream)) return 1;
  if (g_op_ig16 == 1 && !(KpadD & 31)) {
    const ConvKernel k = conv_route(a, -1).k;
    if ((k == kConvIgemm || k == kConvS2Dgrad) && op_ig_bank(wd, Cin, KpadD, 0, (hipStream_t)stream, &a.wbank)) return 1;
  }
  LCHK(launch_conv(a, (hipStream_t)stream));
  return 0;
}
// The dgrad role of the fp16x3 direct kernels (conv_f16x3.hip / conv_f16x3v2.hip), as run_dgrad launches it: ConvArgs of a 3x3 /
// stride-1 / pad-1 input gradient, the bank packed straight from the FORWARD weights (bank job mode 2), max|dY| through a one-off reduction
int uwm_op_dgrad_f16x3(const float* dy, int N, int H, int W, int Cout, int CoutP, const float* w, int Kpad, int Cin,
                       const float* addend, const float* mask, const float* mscale, const float* mshift, const float* bnb_mean,
                       const float* bnb_rstd, const float* bnb_y, double* sums, int nrep, long long sums_stride, float* dx, int cfg,
                       uwm_stream stream) {
  if (!dy || !w || !dx) return fail("uwm_op_dgrad_f16x3: null argument");
  if (cfg == 604 || cfg == 606) return fail("uwm_op_dgrad_f16x3: cfg %d names a removed conv_f16x3v2 form (607 is its kernel)", cfg);
  if (cfg < 600 || cfg > 607) return fail("uwm_op_dgrad_f16x3: cfg must be 600..603, 605 or 607, got %d", cfg);
  if (N < 1 || H < 8 || W < 16 || Cout < 1 || CoutP < Cout || (CoutP & 31) || Cin < 16 || (Cin & 3) || (Kpad & 31) || (long long)Kpad < 9LL * Cin)
    return fail("uwm_op_dgrad_f16x3: needs H >= 8, W >= 16, padded dY channels %% 32 == 0, Cin %% 4 == 0, forward weights [Cout][Kpad >= 9 * Cin] (k = tap * Cin + c)");
  if ((mscale == nullptr) != (mshift == nullptr) || (mscale && !mask)) return fail("uwm_op_dgrad_f16x3: mscale / mshift come together, with a mask");
  if (!bnb_mean && (bnb_rstd || bnb_y)) return fail("uwm_op_dgrad_f16x3: bnb_rstd / bnb_y without bnb_mean");
  if (bnb_mean && (!bnb_rstd || !sums || !(bnb_y || mask))) return fail("uwm_op_dgrad_f16x3: the fused BatchNorm-backward sums need bnb_rstd, a sums buffer and a mask or bnb_y");
  if (sums && (nrep < 1 || (nrep & (nrep - 1)) || (nrep > 1 && (sums_stride < 2LL * Cin || sums_stride > 0x7fffffffLL)))) return fail("uwm_op_dgrad_f16x3: nrep must be a power of two, replicas at least 2 * Cin doubles apart");
  hipStream_t st = (hipStream_t)stream;
  static float* buf = nullptr; static size_t cap = 0;
  static float* xm = nullptr;
  const size_t need = f16x3_bank_floats(Cin, CoutP);
  if (need > cap) {
    HIPCHK(hipDeviceSynchronize());
    if (buf) HIPCHK(hipFree(buf));
    buf = nullptr; cap = 0;
    HIPCHK(hipMalloc((void**)&buf, need * sizeof(float))); cap = need;
  }
  if (!xm) HIPCHK(hipMalloc((void**)&xm, 32 * sizeof(float)));
  const int variant = cfg - 600;
  const int layout = variant >= 4 ? 1 : (variant == 0 && f16x3v2_shape(H, W, Cin, CoutP) ? 1 : 0);      // as op_f16x3_prepare
  ConvArgs a; memset(&a, 0, sizeof(a));
  a.s0 = mk_src(dy, CoutP, H, W); a.s1 = a.s0; a.C0 = CoutP; a.Ctot = CoutP;
  a.w = w; a.wrows = Cin; a.Kpad = Kpad; a.ntaps = 9; a.kw = 3;
  a.N = N; a.Ho = H; a.Wo = W; a.Cout = Cin; a.M = N * H * W;
  a.Hl = H; a.Wl = W; a.smul = 1; a.rmul = -1; a.off = 1; a.sdiv = 1;
  a.out = dx; a.addend = addend; a.mask = mask; a.mscale = mscale; a.mshift = mshift; a.live_ch = Cout;
  a.dv_ctot = make_fastdiv(a.Ctot); a.dv_kw = make_fastdiv(a.kw);
  a.wu = buf; a.wu_layout = layout; a.wu_ncb = layout == 1 ? f16x3v2_nf(Cin) : f16x3_nj(Cin); a.wu_rinv_off = (int)f16x3_rinv_off(Cin, CoutP);
  a.prec = 2; a.nprod = g_op_f3_nprod; a.xmax = xm;
  a.bnb_mean = bnb_mean; a.bnb_rstd = bnb_rstd; a.bnb_y = bnb_y;
  if (sums) { a.ssum = sums; a.ssq = sums + Cin; a.srep = nrep; a.sstride = (int)sums_stride; }
  if (conv_route(a, cfg).k == kConvInvalid) return fail("uwm_op_dgrad_f16x3: cfg %d: the coded fp16x3 kernel does not take this shape", cfg);      // (nothing launched)
  WinoJobs jobs; jobs.n = 1;
  WinoJob& j = jobs.j[0];
  j.w = w; j.ut = buf; j.rows = Cin; j.chans = CoutP; j.Kpad = Kpad; j.mode = 2; j.src_rows = Cout; j.pad_ = layout;
  LCHK(launch_f16x3_weights_multi(jobs, st));
  LCHK(launch_absmax32(dy, (size_t)N * H * W * CoutP, xm, st));
  LCHK(launch_conv(a, st, cfg));
  return 0;
}
int uwm_op_dgrad_upsplit(const float* dy, int N, int H, int W, int Cout, const float* wd, int C0, int C1, int KpadD,
                         float* gprev, const float* pmask, const float* pscale, const float* pshift, float* gskip,
                         uwm_stream stream) {
  if (!dy || !wd || !gprev || (C1 > 0 && !gskip)) return fail("uwm_op_dgrad_upsplit: null argument");
  ConvArgs a; memset(&a, 0, sizeof(a));
  a.s0 = mk_src(dy, Cout, H, W); a.s1 = a.s0; a.C0 = Cout; a.Ctot = Cout;
  a.w = wd; a.wrows = C0 + C1; a.Kpad = KpadD; a.ntaps = 9; a.kw = 3;
  a.N = N; a.Ho = H; a.Wo = W; a.Cout = C0 + C1; a.M = N * H * W;
  a.Hl = H; a.Wl = W; a.smul = 1; a.rmul = -1; a.off = 1; a.sdiv = 1;
  a.out = gskip; a.out_up = gprev; a.up_c0 = C0; a.up_mask = pmask; a.up_mscale = pscale; a.up_mshift = pshift;
  a.dv_ctot = make_fastdiv(a.Ctot); a.dv_kw = make_fastdiv(a.kw);
  if (!op_wino_shape(a, 3, 3, 1, 1) || (H & 1) || (W & 1)) return fail("uwm_op_dgrad_upsplit: needs even H >= 8, W >= 16, channels %% 8 == 0");
  if (g_op_ig16) {                                 // conv_up2_f16.hip's sub-pixel dgrad: max|dy| through a one-off reduction
    static float* xm = nullptr;
    if (!xm) HIPCHK(hipMalloc((void**)&xm, 32 * sizeof(float)));
    LCHK(launch_absmax32(dy, (size_t)N * H * W * Cout, xm, (hipStream_t)stream));
    a.ig16 = 1; a.xmax = xm;
  }
  if (op_wino_prepare(a, 1, (hipStream_t)stream)) return 1;
  LCHK(launch_conv(a, (hipStream_t)stream));
  return 0;
}
int uwm_op_wgrad(const uwm_src* s0, const uwm_src* s1, const float* dy, int N, int Ho, int Wo, int Cout, int wrows, int Kpad,
                 int kh, int kw, int stride, int pad, float* dw, int force_igemm, uwm_stream stream) {
  if (!s0 || !dy || !dw) return fail("uwm_op_wgrad: null argument");
  WgradArgs a; memset(&a, 0, sizeof(a));
  a.s0 = to_src(s0); a.C0 = a.s0.C;
  if (s1) { a.s1 = to_src(s1); a.Ctot = a.C0 + a.s1.C; } else { a.s1 = a.s0; a.Ctot = a.C0; }
  a.dy = dy; a.dw = dw; a.wrows = wrows; a.Kpad = Kpad; a.ntaps = kh * kw; a.kw = kw;
  a.N = N; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout; a.M = N * Ho * Wo;
  a.Hl = a.s0.H << a.s0.up; a.Wl = a.s0.W << a.s0.up; a.stride = stride; a.pad = pad;
  a.dv_ctot = make_fastdiv(a.Ctot); a.dv_kw = make_fastdiv(a.kw);
  a.force_igemm = force_igemm;
  if ((force_igemm & 0xff) == 6 || (force_igemm & 0xff) == 7) {               // fp16x3 weight gradients (6: the direct / dedicated kernels, 7: the flattened implicit GEMM; tests / timing): max|dy| through a one-off reduction
    static float* xm = nullptr;
    if (!xm) HIPCHK(hipMalloc((void**)&xm, 32 * sizeof(float)));
    LCHK(launch_absmax32(dy, (size_t)N * Ho * Wo * Cout, xm, (hipStream_t)stream));
    a.prec = 2; a.nprod = g_op_f3_nprod; a.xmax = xm;      // (nprod: wgrad_f16x3.hip's product count; the other fp16x3 weight-gradient kernels have one form)
  }
  LCHK(launch_wgrad(a, (hipStream_t)stream));
  return 0;
}
int uwm_op_pack_dgrad(const float* w, int Cout, int Kpad, int ntaps, int Cin, float* wd, int KpadD, int CoutP,
                      uwm_stream stream) {
  if (!w || !wd) return fail("uwm_op_pack_dgrad: null argument");
  LCHK(launch_pack_dgrad(w, Cout, Kpad, ntaps, Cin, wd, KpadD, CoutP, (hipStream_t)stream));
  return 0;
}
int uwm_op_bn_backward(const float* g, const float* y, const float* mean, const float* rstd, const float* gamma,
                       double* scratch2c, float* dy, float* dgamma, float* dbeta, long long npix, int C, uwm_stream stream) {
  if (!g || !y || !mean || !rstd || !gamma || !scratch2c || !dy || !dgamma || !dbeta || npix < 1) return fail("uwm_op_bn_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(scratch2c, 0, 2 * (size_t)C * sizeof(double), st));
  LCHK(launch_bn_bwd_reduce(g, y, mean, rstd, scratch2c, scratch2c + C, (size_t)npix, C, st));
  LCHK(launch_bn_bwd_apply(g, y, mean, rstd, gamma, scratch2c, scratch2c + C, dy, dgamma, dbeta, (size_t)npix, C, st));
  return 0;
}
int uwm_op_bn_backward_act(const float* g, const float* y, const float* mean, const float* rstd, const float* gamma,
                           const float* scale, const float* shift, const float* se_s, const float* gpool, int N, long long hw,
                           int C, double* scratch2c, float* dy, float* dgamma, float* dbeta, float* xmax, uwm_stream stream) {
  if (!g || !y || !mean || !rstd || !gamma || !scale || !shift || !scratch2c || !dy || !dgamma || !dbeta || N < 1 || hw < 1 ||
      C < 4 || (C & 3) || (!se_s != !gpool))
    return fail("uwm_op_bn_backward_act: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(scratch2c, 0, 2 * (size_t)C * sizeof(double), st));
  if (xmax) HIPCHK(hipMemsetAsync(xmax, 0, 32 * sizeof(float), st));
  LCHK(launch_bn_bwd_act(g, y, mean, rstd, gamma, scale, shift, se_s, gpool, N, (size_t)hw, scratch2c, scratch2c + C, dy, dgamma,
                         dbeta, C, st, xmax));
  return 0;
}
int uwm_op_upsplit(const float* dcat, int N, int H, int W, int C0, int C1, float* gprev, const float* pmask,
                   const float* pscale, const float* pshift, float* gskip, uwm_stream stream) {
  if (!dcat || !gprev) return fail("uwm_op_upsplit: null argument");
  LCHK(launch_upsplit(dcat, N, H, W, C0, C1, gprev, pmask, pscale, pshift, gskip, (hipStream_t)stream));
  return 0;
}
int uwm_op_residual(const float* y, const float* s2, const float* b2, const float* id, const float* sd, const float* bd,
                    float* out, long long npix, int C, uwm_stream stream) {
  if (!y || !s2 || !b2 || !id || !out) return fail("uwm_op_residual: null argument");
  LCHK(launch_residual(y, s2, b2, id, sd, bd, out, (size_t)npix, C, (hipStream_t)stream));
  return 0;
}
int uwm_op_maxpool_backward(const float* gout, const uint8_t* idx, const float* addend, const uwm_src* in, int N, float* gin,
                            uwm_stream stream) {
  if (!gout || !idx || !in || !gin) return fail("uwm_op_maxpool_backward: null argument");
  Src s = to_src(in);
  LCHK(launch_maxpool_bwd(gout, idx, addend, s, gin, N, (s.H - 1) / 2 + 1, (s.W - 1) / 2 + 1, (hipStream_t)stream));
  return 0;
}
int uwm_op_maxpool(const uwm_src* in, int N, float* out, uint8_t* idx, uwm_stream stream) {
  if (!in || !out) return fail("uwm_op_maxpool: null argument");
  Src s = to_src(in);
  LCHK(launch_maxpool_fwd(s, out, idx, N, (s.H - 1) / 2 + 1, (s.W - 1) / 2 + 1, (hipStream_t)stream));
  return 0;
}

// ---- watermark cut-outs from pairs (extract_u8.hip): every argument is checked here, before any launch
static int extract_caps_check(const char* fn, int N, long long total_pixels, int J) {
  if (N < 0 || J < 0 || (N < 1 && J < 1)) return fail("%s: N and J must be >= 0 and one of them >= 1 (got %d, %d)", fn, N, J);
  if (N > 65535 || J > 65535) return fail("%s: at most 65535 images and 65535 jobs per call (got %d, %d)", fn, N, J);
  if (N >= 1 && (total_pixels < 1 || total_pixels > (1ll << 40))) return fail("%s: total_pixels must be 1 .. 2^40 (got %lld)", fn, total_pixels);
  return 0;
}
size_t uwm_extract_workspace_bytes(int N, long long total_pixels, int J) {
  if (extract_caps_check("uwm_extract_workspace_bytes", N, total_pixels, J)) return 0;
  return extract_workspace_bytes(N, total_pixels, J);
}
int uwm_extract_regions_ragged(const uint8_t* wm, size_t wm_bytes, const uwm_image_desc* wm_descs, const uint8_t* clean, size_t clean_bytes,
                               const uwm_image_desc* clean_descs, int N, int C, int threshold, int min_area, long long max_pixels,
                               long long total_pixels, uint8_t* plane, size_t plane_bytes, const uwm_image_desc* plane_descs, long long* stats,
                               long long* table, void* ws, size_t ws_bytes, uwm_stream stream) {
  const char* fn = "uwm_extract_regions_ragged";
  if (!wm || !wm_descs || !clean || !clean_descs || !plane || !plane_descs || !stats || !table || !ws) return fail("%s: null argument", fn);
  if (C != 3) return fail("%s: C must be 3 (RGB pairs; got %d)", fn, C);
  if (threshold < 0 || threshold > 255) return fail("%s: threshold must be 0..255 (got %d)", fn, threshold);
  if (min_area < 0 || min_area > (1 << 30)) return fail("%s: min_area must be 0 .. 2^30 (got %d)", fn, min_area);
  if (N < 1 || wm_bytes < 1 || clean_bytes < 1 || plane_bytes < 1)
    return fail("%s: N, wm_bytes, clean_bytes and plane_bytes must be >= 1 (got %d, %zu, %zu, %zu)", fn, N, wm_bytes, clean_bytes, plane_bytes);
  if (extract_caps_check(fn, N, total_pixels, 0)) return 1;
  if (((uintptr_t)wm | (uintptr_t)clean) & 3) return fail("%s: wm and clean must be 4-byte aligned", fn);
  if (max_pixels < 1 || max_pixels > (1ll << 30)) return fail("%s: max_pixels must be 1 .. 2^30 (got %lld)", fn, max_pixels);
  if (((uintptr_t)wm_descs | (uintptr_t)clean_descs | (uintptr_t)plane_descs | (uintptr_t)stats | (uintptr_t)table | (uintptr_t)ws) & 7)
    return fail("%s: descriptors, stats, table and the workspace must be 8-byte aligned", fn);
  const size_t need = extract_workspace_bytes(N, total_pixels, 0);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_extract_regions(wm, wm_bytes, (const ImageDesc*)wm_descs, clean, clean_bytes, (const ImageDesc*)clean_descs, N, threshold, min_area,
                              max_pixels, total_pixels, plane, plane_bytes, (const ImageDesc*)plane_descs, stats, table, ws, (hipStream_t)stream));
  return 0;
}
int uwm_extract_cutouts_ragged(const uint8_t* wm, size_t wm_bytes, const uwm_image_desc* wm_descs, const uint8_t* plane, size_t plane_bytes,
                               const uwm_image_desc* plane_descs, int N, const uwm_extract_job* jobs, int J, long long max_crop_pixels,
                               uint8_t* out, size_t out_bytes, int* status, void* ws, size_t ws_bytes, uwm_stream stream) {
  const char* fn = "uwm_extract_cutouts_ragged";
  static_assert(sizeof(uwm_extract_job) == sizeof(ExtractJob) && sizeof(ExtractJob) == 288, "uwm_extract_job layout");
  if (!wm || !wm_descs || !plane || !plane_descs || !jobs || !out || !status || !ws) return fail("%s: null argument", fn);
  if (N < 1 || J < 1 || wm_bytes < 1 || plane_bytes < 1 || out_bytes < 1)
    return fail("%s: N, J, wm_bytes, plane_bytes and out_bytes must be >= 1 (got %d, %d, %zu, %zu, %zu)", fn, N, J, wm_bytes, plane_bytes, out_bytes);
  if (extract_caps_check(fn, 0, 0, J)) return 1;
  if (max_crop_pixels < 1 || max_crop_pixels > (1ll << 30)) return fail("%s: max_crop_pixels must be 1 .. 2^30 (got %lld)", fn, max_crop_pixels);
  if (((uintptr_t)wm | (uintptr_t)out) & 3) return fail("%s: wm and out must be 4-byte aligned", fn);
  if ((uintptr_t)status & 3) return fail("%s: status must be 4-byte aligned", fn);
  if (((uintptr_t)wm_descs | (uintptr_t)plane_descs | (uintptr_t)jobs | (uintptr_t)ws) & 7)
    return fail("%s: descriptors, jobs and the workspace must be 8-byte aligned", fn);
  const size_t need = extract_workspace_bytes(0, 0, J);
  if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
  LCHK(launch_extract_cutouts(wm, wm_bytes, (const ImageDesc*)wm_descs, plane, plane_bytes, (const ImageDesc*)plane_descs, N,
                              (const ExtractJob*)jobs, J, max_crop_pixels, out, out_bytes, status, ws, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
