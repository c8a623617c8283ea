// libuwm, part of uwm_model.hip (one translation unit; included from there): launch helpers: ConvArgs / WgradArgs of a layer's forward, dgrad, wgrad, BatchNorm passes; filter-bank jobs; the routing record.
// ------------------------------------------------------------------------------ launch helpers
struct Ctx {
  uwm_model* m; float* ws; hipStream_t st; int N;
  hipStream_t wst = nullptr;          // stream for wgrad launches (== st when the side stream is off)
  float* fz = nullptr;                // frozen arena, when this (eval) forward reads it (frozen_serves); null = everything in the workspace
  float* F(size_t off) const { return ws + off; }
  // the one place that decides "arena or workspace": a BatchNorm's {scale[C], shift[C]} and a conv's forward bank
  const float* bn_ss(const BNL& b) const { return fz ? fz + b.fz_off : ws + b.f_off + 2 * b.C; }
  float* wu(const ConvL& cv) const { return fz ? fz + cv.fz_wu : ws + cv.wu_off; }
  double* D(size_t doff) const { return (double*)ws + doff; }
};
static Src mk_src(const float* ptr, int C, int H, int W, const float* scale = nullptr, const float* shift = nullptr,
                  int relu = 0, int up = 0) {
  Src s; s.ptr = ptr; s.scale = scale; s.shift = shift; s.C = C; s.H = H; s.W = W; s.up = up; s.relu = relu; return s;
}
static Src lazy_src(const Ctx& c, int conv, int H, int W, int relu = 1, int up = 0) {
  const ConvL& cv = c.m->convs[conv];
  const BNL& b = c.m->bns[cv.bn];
  return mk_src(c.F(c.m->plan.y[conv]), cv.CoutP, H, W, c.bn_ss(b), c.bn_ss(b) + b.C, relu, up);
}

// a launch helper that found a contract violation of its own: the message is set here and LCHK passes it on unchanged
static thread_local bool g_err_own = false;
static hipError_t fail_launch(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
  g_err_own = true;
  return hipErrorInvalidValue;
}

// The max|dY| contract of the fp16x3 backward.  Every fp16x3 dgrad / wgrad of conv ci stages dY times the power of two that
// puts max|dY| into [2^13, 2^14); it reads that maximum from the 32 slots of the conv's BatchNorm (BNL::xmax_off), which the
// BatchNorm backward that writes dY fills (run_bn_bwd, run_bn_bwd_act).  An unwritten slot reads 0 and the kernels fall back to
// scale 1 without a word (dY below ~6e-5 loses mantissa, below ~6e-8 flushes to zero).  The producers write the slots of every
// conv this predicate holds for; it is the OR of the very functions run_dgrad (f3_dgrad_on, conv_ig16) and run_wgrad (wgrad_f16_on)
// switch their launch to fp16x3 by, and those read the slots only through dy_max_slot: no consumer without a producer.
static bool dy_max_needed(const uwm_model* m, size_t ci) {
  return m->convs[ci].bn >= 0 && (f3_dgrad_on(m, ci) || conv_ig16(m, ci, true) || wgrad_f16_on(m, ci));
}
// *slot = the max|dY| slots an fp16x3 dgrad / wgrad of conv ci reads; an error when no producer of this backward wrote them (a
// new fp16x3 route without a producer fails here instead of silently running on unscaled fp16)
static hipError_t dy_max_slot(const Ctx& c, int ci, const char* pass, const float** slot) {
  const ConvL& cv = c.m->convs[ci];
  if (!dy_max_needed(c.m, (size_t)ci) || cv.bn >= (int)c.m->dy_max_made.size() || !c.m->dy_max_made[cv.bn])
    return fail_launch("internal: the fp16x3 %s of %s has no max|dY| producer (dy_max_needed / run_bn_bwd*)", pass, cv.name.c_str());
  *slot = (const float*)c.D(c.m->bns[cv.bn].xmax_off());
  return hipSuccess;
}

// routing record (uwm_routing_enable / uwm_routing_dump): "<pass> <layer> <kernel>" per conv-class launch, in launch order
static hipError_t route_rec(const Ctx& c, const char* pass, int ci, hipError_t e) {
  if (c.m->route_log_on && e == hipSuccess) { c.m->route_log += pass; c.m->route_log += ' '; c.m->route_log += c.m->convs[ci].name; c.m->route_log += ' '; c.m->route_log += route_last(); c.m->route_log += '\n'; }
  return e;
}

static hipError_t run_conv_fwd(const Ctx& c, int ci, const Src& s0, const Src* s1, int Ho, int Wo, float* out,
                               bool stats, int cfg = -1) {
  const ConvL& cv = c.m->convs[ci];
  ConvArgs a; memset(&a, 0, sizeof(a));
  a.s0 = s0; a.C0 = s0.C;
  if (s1) { a.s1 = *s1; a.Ctot = s0.C + s1->C; } else { a.s1 = s0; a.Ctot = s0.C; }
  a.w = c.m->params + cv.w_off; a.wrows = cv.Cout; a.Kpad = cv.Kpad; a.ntaps = cv.k * cv.k; a.kw = cv.k;
  a.N = c.N; a.Ho = Ho; a.Wo = Wo; a.Cout = cv.CoutP; a.M = c.N * Ho * Wo;
  a.Hl = s0.H << s0.up; a.Wl = s0.W << s0.up;
  a.smul = cv.stride; a.rmul = 1; a.off = -cv.pad; a.sdiv = 1;
  a.out = out; a.bias = cv.bias_off >= 0 ? c.m->params + cv.bias_off : nullptr;
  if (stats && cv.bn >= 0) {
    const BNL& b = c.m->bns[cv.bn];
    a.ssum = c.D(b.d_off) + 2 * b.C; a.ssq = a.ssum + b.C; a.srep = b.nrep; a.sstride = 2 * b.C;
  }
  a.dv_ctot = make_fastdiv(a.Ctot); a.dv_kw = make_fastdiv(a.kw);
  a.flops = 2.0 * (double)a.M * cv.Cout * cv.Cin * cv.k * cv.k;
  a.bytes = 4.0 * ((double)c.N * s0.H * s0.W * s0.C + (s1 ? (double)c.N * s1->H * s1->W * s1->C : 0.0) + (double)cv.Cout * cv.Kpad +
                   (double)a.M * cv.CoutP);
  if (ci == c.m->stem && cfg < 0 && stem_f3_on(c.m)) {
    a.wu = c.wu(cv);
    if (conv_stem_f16x3_applicable(a)) return route_rec(c, "fwd", ci, launch_conv_stem_f16x3(a, c.st));
    a.wu = nullptr;
  }
  if (cv.wu_off && !cv.stem7() && !cv.igb() && a.Ctot == cv.CinP && c.m->plan.wino_ok((size_t)ci)) {
    a.wu = c.wu(cv); a.wu_ncb = wino_ncb(cv.Cout);
    if (c.m->plan.prec == UWM_PREC_BF16X3_ALL && cv.x3()) {
      if (a.C0 != cv.c0 && a.C0 != a.Ctot) return hipErrorInvalidValue;       // the bank was split for this concat boundary
      a.prec = 1;
    }
    if (f3_fwd_on(c.m, (size_t)ci)) {
      a.prec = 2; a.wu_layout = f3_layout(c.m, (size_t)ci, false); a.nprod = f3_nprod(c.m, false);
      a.wu_ncb = a.wu_layout == 1 ? f16x3v2_nf(cv.Cout) : f16x3_nj(cv.Cout); a.wu_rinv_off = (int)f16x3_rinv_off(cv.Cout, cv.CinP);
    }
  }
  a.wino = c.m->plan.wino_mode + 1; a.route_n = c.m->route_n;
  if (conv_ig16(c.m, (size_t)ci, false)) a.ig16 = 1;
  if (ig_bank_on(c.m, (size_t)ci, false) && a.Ctot == cv.CinP && cfg < 0) a.wbank = c.wu(cv);
  return route_rec(c, "fwd", ci, launch_conv(a, c.st, cfg));
}

struct UpSplit { float* gprev; int C0; const float* pmask; const float* pscale; const float* pshift; int accumulate = 0; };
// dX = dgrad(dY) (+addend) (*mask); with `us`: decoder concat split fused into the epilogue (dx = gskip or nullptr)
// bn_fuse >= 0: the masked output of this dgrad is the gradient wrt the output of BatchNorm `bn_fuse`, whose raw input is the
// ReLU mask the epilogue reads anyway: where the launch runs on a Winograd epilogue the BatchNorm-backward sums (dbeta,
// dgamma partials, one of nrep replicas per workgroup) are accumulated there and *fused = true tells run_bn_bwd to skip
// its reduce pass.  bn_y: yhat comes from this tensor instead of the mask tensor (gradient wrt a residual block's output: masked by the
// output, but the BatchNorm in question is the block's last one, whose raw input is bn_y)
static hipError_t run_dgrad(const Ctx& c, int ci, const float* dy, int Ho, int Wo, int Hin, int Win, float* dx,
                            const float* addend, const float* mask, const float* mscale, const float* mshift,
                            const UpSplit* us = nullptr, int bn_fuse = -1, bool* fused = nullptr, const float* bn_y = nullptr) {
  const ConvL& cv = c.m->convs[ci];
  ConvArgs a; memset(&a, 0, sizeof(a));
  a.s0 = mk_src(dy, cv.CoutP, Ho, Wo); a.s1 = a.s0; a.C0 = cv.CoutP; a.Ctot = cv.CoutP;
  a.w = c.F(cv.wd_off); a.wrows = cv.CinP; a.Kpad = cv.KpadD; a.ntaps = cv.k * cv.k; a.kw = cv.k;
  a.N = c.N; a.Ho = Hin; a.Wo = Win; a.Cout = cv.CinP; a.M = c.N * Hin * Win;
  a.Hl = Ho; a.Wl = Wo; a.smul = 1; a.rmul = -1; a.off = cv.pad; a.sdiv = cv.stride;
  a.out = dx; a.addend = addend; a.mask = mask; a.mscale = mscale; a.mshift = mshift; a.live_ch = cv.Cout;
  a.dv_ctot = make_fastdiv(a.Ctot); a.dv_kw = make_fastdiv(a.kw);
  a.flops = 2.0 * (double)c.N * Ho * Wo * cv.Cout * cv.Cin * cv.k * cv.k;   // same MACs as the forward conv
  a.bytes = 4.0 * ((double)c.N * Ho * Wo * cv.CoutP + (double)cv.CinP * cv.KpadD +
                   (double)a.M * cv.CinP * (1.0 + (addend ? 1.0 : 0.0) + (mask ? 1.0 : 0.0)));
  if (cv.wud_off && c.m->plan.wino_ok((size_t)ci)) {
    a.wu = c.F(cv.wud_off); a.wu_ncb = wino_ncb(cv.CinP);
    const int pm = c.m->plan.prec;
    if ((pm == UWM_PREC_BF16X3 || pm == UWM_PREC_BF16X3_ALL) && cv.x3_d()) a.prec = 1;
    if (f3_dgrad_on(c.m, (size_t)ci)) {        // fp16x3 direct form (a concat boundary sits on a 64-channel tile: f3d_plain)
      a.prec = 2; a.wu_layout = f3_layout(c.m, (size_t)ci, true); a.nprod = f3_nprod(c.m, true);
      a.wu_ncb = a.wu_layout == 1 ? f16x3v2_nf(cv.CinP) : f16x3_nj(cv.CinP); a.wu_rinv_off = (int)f16x3_rinv_off(cv.CinP, cv.CoutP);
    }
  }
  a.wino = c.m->plan.wino_mode + 1;
  if (conv_ig16(c.m, (size_t)ci, true)) a.ig16 = 1;
  if (ig_bank_on(c.m, (size_t)ci, true)) a.wbank = c.F(cv.wdb_off);
  if (a.prec == 2 || a.ig16) {                 // dY scaled by the power of two bn_bwd_apply's max|dy| calls for
    const hipError_t e = dy_max_slot(c, ci, "dgrad", &a.xmax);
    if (e != hipSuccess) return e;
  }
  if (us) { a.out_up = us->gprev; a.up_c0 = us->C0; a.up_mask = us->pmask; a.up_mscale = us->pscale; a.up_mshift = us->pshift; a.up_accum = us->accumulate; }
  if (fused) *fused = false;
  static const bool no_fuse = dbg_flag("UWM_NO_BN_FUSE");
  a.bnb_y = bn_y;                                  // (consulted by conv_epilogue_carries_bnb; cleared again when the sums are not fused)
  if (bn_fuse >= 0 && fused && !no_fuse && (us ? (us->pmask != nullptr && !us->accumulate) : (mask != nullptr || bn_y != nullptr)) && conv_epilogue_carries_bnb(a)) {
    const BNL& b = c.m->bns[bn_fuse];
    if (b.C == (us ? us->C0 : cv.CinP)) {
      const float* f = c.F(b.f_off);
      a.bnb_mean = f; a.bnb_rstd = f + b.C;
      a.ssum = c.D(b.d_off) + 2 * b.C; a.ssq = a.ssum + b.C; a.srep = b.nrep; a.sstride = 2 * b.C;     // the forward's (dead, re-zeroed) replicas
      *fused = true;
    }
  }
  if (!fused || !*fused) a.bnb_y = nullptr;
  a.route_n = c.m->route_n;
  return route_rec(c, "dgrad", ci, launch_conv(a, c.st));
}

static hipError_t run_wgrad(const Ctx& c, int ci, const Src& s0, const Src* s1, const float* dy, int Ho, int Wo) {
  const ConvL& cv = c.m->convs[ci];
  WgradArgs a; memset(&a, 0, sizeof(a));
  a.s0 = s0; a.C0 = s0.C;
  if (s1) { a.s1 = *s1; a.Ctot = s0.C + s1->C; } else { a.s1 = s0; a.Ctot = s0.C; }
  a.dy = dy; a.dw = c.m->grads + cv.w_off; a.wrows = cv.Cout; a.Kpad = cv.Kpad; a.ntaps = cv.k * cv.k; a.kw = cv.k;
  a.N = c.N; a.Ho = Ho; a.Wo = Wo; a.Cout = cv.CoutP; a.M = c.N * Ho * Wo;
  a.Hl = s0.H << s0.up; a.Wl = s0.W << s0.up; a.stride = cv.stride; a.pad = cv.pad;
  a.dv_ctot = make_fastdiv(a.Ctot); a.dv_kw = make_fastdiv(a.kw);
  a.flops = 2.0 * (double)a.M * cv.Cout * cv.Cin * cv.k * cv.k;
  a.bytes = 4.0 * ((double)a.M * cv.CoutP + (double)c.N * s0.H * s0.W * s0.C + (s1 ? (double)c.N * s1->H * s1->W * s1->C : 0.0) +
                   (double)cv.Cout * cv.Kpad);
  a.wino = c.m->plan.wino_mode + 1; a.route_n = c.m->route_n;
  if (f3_wgrad_on(c.m, (size_t)ci)) { a.nprod = f3_nprod(c.m, true); a.cu_share = (c.wst && c.wst != c.st) ? 3 : 0; }
  if (wgrad_f16_on(c.m, (size_t)ci)) {
    a.prec = 2;
    const hipError_t e = dy_max_slot(c, ci, "wgrad", &a.xmax);
    if (e != hipSuccess) return e;
  }
  // partial images of a split launch: the next free slice of the scratch; their reduce is queued and runs with the other layers'
  // in one launch (flush_reduces: when the scratch / queue fills up and at the end of every backward stage)
  static const bool no_defer = dbg_flag("UWM_NO_DEFER_REDUCE");
  ReduceQueue& rq = c.m->rq;
  const size_t cap = wgrad_wino_scratch_floats();
  if (rq.n + 1 >= ReduceQueue::kMax || rq.used_floats + cap > kWgParts * cap) {
    hipError_t e = launch_wgrad_reduce_multi(rq, (c.wst && c.wst != c.st) ? c.wst : c.st);
    if (e != hipSuccess) return e;
  }
  a.part = c.F(c.m->plan.wg_part) + rq.used_floats; a.part_floats = cap; a.rq = no_defer ? nullptr : &rq;
  if (c.wst && c.wst != c.st) {
    // fork: the side stream must see everything enqueued so far on the main stream (dy, activations).  Where dy came out of a
    // bn_bwd_apply dispatch that carried ev_disp, that event IS the fork point
    const bool covered = std::find(c.m->disp_cov.begin(), c.m->disp_cov.end(), dy) != c.m->disp_cov.end();
    hipError_t e = hipSuccess;
    if (!covered) e = hipEventRecord(c.m->ev_fork, c.st);
    if (e != hipSuccess) return e;
    e = hipStreamWaitEvent(c.wst, covered ? c.m->ev_disp : c.m->ev_fork, 0);
    if (e != hipSuccess) return e;
    return route_rec(c, "wgrad", ci, launch_wgrad(a, c.wst));
  }
  return route_rec(c, "wgrad", ci, launch_wgrad(a, c.st));
}

static hipError_t run_bn_finalize(const Ctx& c, int bi, size_t count, int training) {
  uwm_model* m = c.m; const BNL& b = m->bns[bi];
  float* f = c.F(b.f_off);
  const float eps = b.eps > 0.f ? b.eps : m->desc.bn_eps, mom = b.mom > 0.f ? b.mom : m->desc.bn_momentum;
  if (training)
    return launch_bn_finalize(c.D(b.d_off) + 2 * b.C, c.D(b.d_off) + 3 * b.C, m->params + b.g_off, m->params + b.b_off,
                              m->buffers + b.rm_off, m->buffers + b.rv_off, f, f + b.C, f + 2 * b.C, f + 3 * b.C, b.C,
                              (double)count, eps, mom, 1, c.st, b.nrep, 2 * b.C);
  ++m->prep_launches;
  return launch_bn_eval(m->params + b.g_off, m->params + b.b_off, m->buffers + b.rm_off, m->buffers + b.rv_off,
                        f + 2 * b.C, f + 3 * b.C, b.C, eps, c.st);
}

// g (masked grad wrt BN output) -> dy ; also writes gamma/beta gradients
static hipError_t run_bn_bwd(const Ctx& c, int ci, const float* g, float* dy, size_t npix, bool sums_fused = false) {
  uwm_model* m = c.m; const ConvL& cv = m->convs[ci]; const BNL& b = m->bns[cv.bn];
  const float* f = c.F(b.f_off); const float* y = c.F(m->plan.y[ci]);
  double* dg = c.D(b.d_off); double* db = c.D(b.d_off) + b.C;
  // sums_fused: the dgrad that produced g left per-workgroup-replica partial sums behind (run_dgrad bn_fuse): the apply pass adds
  // the replicas up in its own prologue (no fold launch between the dgrad and the apply)
  hipEvent_t done = nullptr;
  if (c.wst && c.wst != c.st && m->ev_disp && m->disp_fork) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c.st, &cs) != hipSuccess) { cs = hipStreamCaptureStatusNone; (void)hipGetLastError(); }
    if (cs == hipStreamCaptureStatusNone) done = m->ev_disp;          // (a capturing stream takes the plain record / wait pair: graph edges)
  }
  hipError_t e = hipSuccess;
  float* xmax = dy_max_needed(m, (size_t)ci) ? (float*)c.D(b.xmax_off()) : nullptr;      // the fp16x3 dgrad / wgrad of this conv scale dy by its maximum
  if (sums_fused)
    e = launch_bn_bwd_apply(g, y, f, f + b.C, m->params + b.g_off, nullptr, nullptr, dy, m->grads + b.g_off, m->grads + b.b_off,
                            npix, b.C, c.st, c.D(b.d_off) + 2 * b.C, b.nrep, 2 * b.C, done, xmax);
  else {
    e = launch_bn_bwd_reduce(g, y, f, f + b.C, dg, db, npix, b.C, c.st);
    if (e != hipSuccess) return e;
    e = launch_bn_bwd_apply(g, y, f, f + b.C, m->params + b.g_off, dg, db, dy, m->grads + b.g_off, m->grads + b.b_off,
                            npix, b.C, c.st, nullptr, 0, 0, done, xmax);
  }
  if (e == hipSuccess && done) m->disp_cov.push_back(dy);
  if (e == hipSuccess && xmax) m->dy_max_made[cv.bn] = 1;
  return e;
}

// BatchNorm backward of conv ci whose output went through swish [and the SE product]: g = grad wrt that activation
static hipError_t run_bn_bwd_act(const Ctx& c, int ci, const float* g, float* dy, int N, size_t hw, const float* se_s, const float* gpool) {
  uwm_model* m = c.m; const ConvL& cv = m->convs[ci]; const BNL& b = m->bns[cv.bn];
  const float* f = c.F(b.f_off);
  float* xmax = dy_max_needed(m, (size_t)ci) ? (float*)c.D(b.xmax_off()) : nullptr;      // (the MBConv expand convs: 1x1 fp16x3 forms)
  const hipError_t e = launch_bn_bwd_act(g, c.F(m->plan.y[ci]), f, f + b.C, m->params + b.g_off, f + 2 * b.C, f + 3 * b.C, se_s, gpool,
                                         N, hw, c.D(b.d_off), c.D(b.d_off) + b.C, dy, m->grads + b.g_off, m->grads + b.b_off, b.C, c.st, xmax);
  if (e == hipSuccess && xmax) m->dy_max_made[cv.bn] = 1;
  return e;
}

#define LCHK(expr)                                                                                     \
  do { hipError_t e_ = (expr); if (e_ != hipSuccess) { if (g_err_own) { g_err_own = false; return 1; }     \
       return fail("launch failed: %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #expr); } } while (0)

// Winograd filter transforms of every eligible layer (forward banks, or dgrad banks straight from the forward
// weights), at most WinoJobs::kMax layers per launch
// (forward banks go where Ctx::wu points: the workspace, or the frozen arena when uwm_freeze fills it)
// (+ the pre-split weight operands of the implicit GEMM's fp16x3 form, ig_bank_on: jobs of the fp16x3 bank launch — the forward
// ones from the parameters, the dgrad ones from the [Cin][tap][Cout] repacks enqueued on this stream before this call)
static hipError_t wino_jobs(const Ctx& c, bool dgrad, hipStream_t st) {
  uwm_model* m = c.m;
  const bool wino_on = m->plan.wino_mode != 0;
  // three passes: fp32 banks, then (bf16x3 modes) the split-bf16 banks of the layers that run on conv_wino_x3, then (fp16x3
  // modes) the split-fp16 banks of the layers that run on conv_f16x3
  const int prec = m->plan.prec;
  const bool bf = prec == UWM_PREC_BF16X3 || prec == UWM_PREC_BF16X3_ALL;
  for (int x3 = wino_on ? 0 : 2; x3 <= 2; ++x3) {
    WinoJobs jobs; jobs.n = 0;
    auto flush = [&]() { if (jobs.n > 0 && !dgrad) ++m->prep_launches; hipError_t e = x3 == 2 ? launch_f16x3_weights_multi(jobs, st) : (x3 ? launch_wino_weights_x3_multi(jobs, st) : launch_wino_weights_multi(jobs, st)); jobs.n = 0; return e; };
    for (size_t ci = 0; ci < m->convs.size(); ++ci) {
      const ConvL& cv = m->convs[ci];
      if (x3 == 2 && ig_bank_on(m, ci, dgrad)) {
        WinoJob& j = jobs.j[jobs.n++];
        j.chans = 0; j.mode = 3; j.pad_ = 0;
        if (dgrad) { j.w = c.F(cv.wd_off); j.ut = c.F(cv.wdb_off); j.rows = cv.CinP; j.Kpad = cv.KpadD; j.src_rows = cv.CinP; }
        else { j.w = m->params + cv.w_off; j.ut = c.wu(cv); j.rows = cv.Cout; j.Kpad = cv.Kpad; j.src_rows = cv.Cout; }
        if (jobs.n == WinoJobs::kMax) { hipError_t e = flush(); if (e != hipSuccess) return e; }
        continue;
      }
      if (!wino_on || cv.igb() || !m->plan.wino_ok(ci) || !(dgrad ? cv.wud_off : cv.wu_off) || cv.stem7()) continue;      // (the stem's slot holds conv_stem_f16x3's bank, built by its own kernel)
      int kind = 0;
      if (dgrad) { if (bf && cv.x3_d()) kind = 1; if (f3_dgrad_on(m, ci)) kind = 2; }
      else { if (prec == UWM_PREC_BF16X3_ALL && cv.x3()) kind = 1; if (f3_fwd_on(m, ci)) kind = 2; }
      if (kind != x3) continue;
      WinoJob& j = jobs.j[jobs.n++];
      j.w = m->params + cv.w_off; j.Kpad = cv.Kpad; j.pad_ = kind == 2 ? f3_layout(m, ci, dgrad) : 0;
      if (dgrad) { j.ut = c.F(cv.wud_off); j.rows = cv.CinP; j.chans = cv.CoutP; j.mode = 2; j.src_rows = cv.Cout; }
      else { j.ut = c.wu(cv); j.rows = cv.Cout; j.chans = cv.CinP; j.mode = 0; j.src_rows = cv.Cout; }
      if (jobs.n == WinoJobs::kMax) { hipError_t e = flush(); if (e != hipSuccess) return e; }
    }
    hipError_t e = flush();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
