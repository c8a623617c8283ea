// libuwm, part of uwm_model.hip (one translation unit; included from there): uwm_forward: the encoder / decoder walk.
// ------------------------------------------------------------------------------ forward
// the stem bank builder where the handle's modes put the stem on conv_stem_f16x3 (into Ctx::wu: workspace, or the frozen arena from uwm_freeze)
static int stem_bank_job(const Ctx& c, hipStream_t st) {
  uwm_model* m = c.m;
  if (!stem_f3_on(m)) return 0;
  const ConvL& sv = m->convs[m->stem];
  ++m->prep_launches;
  LCHK(launch_stem_f16x3_weights(m->params + sv.w_off, sv.Kpad, sv.CinP, c.wu(sv), st));
  return 0;
}
// x == nullptr: the caller has filled plan.x4 (the NHWC4 input) itself (uwm_predict_u8)
static int do_forward(uwm_model* m, const float* x, float* logits, float* ws, int N, int H, int W, int training,
                      hipStream_t st) {
  const Plan& p = m->plan;
  Ctx c{m, ws, st, N};
  if (training) m->frozen = nullptr;          // the running statistics move: what the arena holds is stale after this call
  // frozen handle, and every layer's bank form for this shape is the frozen one: scale / shift and banks come from the arena and no
  // preparation kernel is launched; else today's path, in the workspace (the arena is written by uwm_freeze alone)
  const bool fz = !training && frozen_serves(m);
  if (fz) c.fz = m->frozen;
  if (m->prec_from_env) {               // say once which arithmetic a process default switched on (a stray variable must not go unnoticed)
    static const char* names[7] = {"f32", "bf16x3", "bf16x3_all", "f16x3", "f16x3_all", "f16x1", "f16x3_bwd2"};
    fprintf(stderr, "libuwm: precision mode %s for this handle comes from UWM_PRECISION (uwm_set_precision overrides it)\n", names[m->prec]);
    m->prec_from_env = false;
  }
  // a previous training forward that was never followed by a backward left its dgrad repacks on the side stream with
  // nothing joined to them: this stream must not touch the workspace (re-planned, re-used or re-allocated) before they land
  if (m->packed_in_fwd) HIPCHK(hipStreamWaitEvent(st, m->ev_pack, 0));
  if (training) HIPCHK(hipMemsetAsync(c.D(p.stat_d), 0, p.stat_d_count * sizeof(double), st));
  m->packed_in_fwd = false;
  if (training && m->use_side && m->side && m->grads) {
    // the [Cin][tap][Cout] weight repacks the backward's dgrads need depend only on the parameters: enqueue them
    // on the side stream now (after everything already on the caller's stream, i.e. after the last optimizer step)
    // so they cost nothing; uwm_backward waits for ev_pack
    HIPCHK(hipEventRecord(m->ev_fork, st));
    HIPCHK(hipStreamWaitEvent(m->side, m->ev_fork, 0));
    for (size_t ci = 0; ci < m->convs.size(); ++ci) {
      const ConvL& cv = m->convs[ci];
      if (cv.dgrad && (!(cv.wud_off && p.wino_ok(ci)) || cv.CoutP == 16 || c16_f16_on(m, ci, true)))      // Winograd dgrads take their filters from wino_jobs below; 16-channel dY goes to conv_patch16 (packed bank), conv_c16_f16.hip's dgrads read the packed filter too
        LCHK(launch_pack_dgrad(m->params + cv.w_off, cv.Cout, cv.Kpad, cv.k * cv.k, cv.CinP, c.F(cv.wd_off), cv.KpadD,
                               cv.CoutP, m->side));
    }
    LCHK(wino_jobs(c, true, m->side));
    HIPCHK(hipEventRecord(m->ev_pack, m->side));
    m->packed_in_fwd = true; m->pack_mode = pack_key(m);
  }
  if (!fz) { LCHK(wino_jobs(c, false, st)); if (stem_bank_job(c, st)) return 1; }
  if (x) LCHK(launch_nchw_to_nhwc4(x, c.F(p.x4), N, m->desc.in_channels, H, W, m->CinP, st));
  // eval: all BN scale/shift come from running stats and are known up front
  if (!training && !fz) for (size_t i = 0; i < m->bns.size(); ++i) LCHK(run_bn_finalize(c, (int)i, 1, 0));
  auto conv_bn_on = [&](const Ctx& cc, int ci, const Src& s0, const Src* s1, int Ho, int Wo) -> int {
    LCHK(run_conv_fwd(cc, ci, s0, s1, Ho, Wo, cc.F(p.y[ci]), training != 0));
    if (training) LCHK(run_bn_finalize(cc, m->convs[ci].bn, (size_t)N * Ho * Wo, 1));
    return 0;
  };
  auto conv_bn = [&](int ci, const Src& s0, const Src* s1, int Ho, int Wo) -> int { return conv_bn_on(c, ci, s0, s1, Ho, Wo); };
  // the downsample branch of a stage's first block (1x1 / stride 2 + BatchNorm) depends only on the block's input: it runs on the
  // side stream beside conv1 / conv2 of the block and joins in front of the residual add (two independent convolutions overlap
  // each other's prologue / epilogue: scripts/overlap_probe.py)
  static const bool no_cd_side = dbg_flag("UWM_NO_SIDE_DOWNSAMPLE");
  // (training only: +0.4 % on the bs16 step; the bs64 eval forward LOSES 1.5 % with it — 4746 vs 4818 img/s — its launches fill the chip alone)
  const bool cd_side = training && !no_cd_side && m->use_side && m->side && m->ev_fork && m->ev_join;
  int h = H / 2, w = W / 2;
  Src x4 = mk_src(c.F(p.x4), m->CinP, H, W);
  if (conv_bn(m->stem, x4, nullptr, h, w)) return 1;
  Src f1 = lazy_src(c, m->stem, h, w);
  const int h1 = h, w1 = w;
  Src feats[4];
  if (m->mb.empty()) {
  h /= 2; w /= 2;
  LCHK(launch_maxpool_fwd(f1, c.F(p.pool), training ? (uint8_t*)c.F(p.pool_idx) : nullptr, N, h, w, st));
  Src cur = mk_src(c.F(p.pool), 64, h, w);
  size_t bi = 0;
  for (int s = 0; s < 4; ++s) {
    for (auto& bl : m->stages[s]) {
      const int ho = h / bl.stride, wo = w / bl.stride;
      const bool cd_aside = bl.cd >= 0 && cd_side;
      if (cd_aside) {
        HIPCHK(hipEventRecord(m->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(m->side, m->ev_fork, 0));
        Ctx cs = c; cs.st = m->side;
        if (conv_bn_on(cs, bl.cd, cur, nullptr, ho, wo)) return 1;
        HIPCHK(hipEventRecord(m->ev_join, m->side));
      }
      if (bl.c3 < 0) {
        if (conv_bn(bl.c1, cur, nullptr, ho, wo)) return 1;
        Src a1 = lazy_src(c, bl.c1, ho, wo);
        if (conv_bn(bl.c2, a1, nullptr, ho, wo)) return 1;
      } else {
        if (conv_bn(bl.c1, cur, nullptr, h, w)) return 1;
        Src a1 = lazy_src(c, bl.c1, h, w);
        if (conv_bn(bl.c2, a1, nullptr, ho, wo)) return 1;
        Src a2 = lazy_src(c, bl.c2, ho, wo);
        if (conv_bn(bl.c3, a2, nullptr, ho, wo)) return 1;
      }
      const int lc = bl.last();
      const BNL& b2 = m->bns[m->convs[lc].bn];
      const float *idp = cur.ptr, *sd = nullptr, *bd = nullptr;
      if (bl.cd >= 0) {
        if (cd_aside) HIPCHK(hipStreamWaitEvent(st, m->ev_join, 0));
        else if (conv_bn(bl.cd, cur, nullptr, ho, wo)) return 1;
        const BNL& bdn = m->bns[m->convs[bl.cd].bn];
        idp = c.F(p.y[bl.cd]); sd = c.bn_ss(bdn); bd = sd + bdn.C;
      }
      LCHK(launch_residual(c.F(p.y[lc]), c.bn_ss(b2), c.bn_ss(b2) + b2.C, idp, sd, bd,
                           c.F(p.xn[bi]), (size_t)N * ho * wo, bl.Cout, st));
      h = ho; w = wo;
      cur = mk_src(c.F(p.xn[bi]), bl.Cout, h, w);
      ++bi;
    }
    feats[s] = cur;
  }
  } else {
    // ---- EfficientNet encoder: every stage of an MBConv block materialised (round-1 correctness-first path)
    auto bn_ss = [&](int ci, const float** sc, const float** sh_) { const BNL& b = m->bns[m->convs[ci].bn]; *sc = c.bn_ss(b); *sh_ = *sc + b.C; };
    const float *sc, *sf;
    bn_ss(m->stem, &sc, &sf);
    LCHK(launch_swish_fwd(c.F(p.y[m->stem]), sc, sf, m->f1C, c.F(p.stem_a), (size_t)N * h * w, st));
    f1 = mk_src(c.F(p.stem_a), m->f1C, h, w);
    m->keep_fwd = training ? m->keep : nullptr;
    Src cur = f1;
    for (size_t bi = 0; bi < m->mb.size(); ++bi) {
      const MBL& b = m->mb[bi];
      const int ho = h / b.stride, wo = w / b.stride;
      if (ho != p.mh[bi] || wo != p.mw[bi]) return fail("internal: MBConv block %d plan mismatch", (int)bi);
      const float* dwin = cur.ptr;
      if (b.ce >= 0) {
        if (conv_bn(b.ce, cur, nullptr, h, w)) return 1;
        bn_ss(b.ce, &sc, &sf);
        LCHK(launch_swish_fwd(c.F(p.y[b.ce]), sc, sf, b.mid, c.F(p.a0[bi]), (size_t)N * h * w, st));
        dwin = c.F(p.a0[bi]);
      }
      const ConvL& dw = m->convs[b.cdw];
      const size_t npo = (size_t)N * ho * wo;
      LCHK(launch_dw_fwd(dwin, m->params + dw.w_off, b.k, b.stride, b.pb, N, h, w, b.mid, ho, wo, c.F(p.y[b.cdw]), st));
      if (training) {
        const BNL& b1 = m->bns[dw.bn];
        LCHK(launch_colstats(c.F(p.y[b.cdw]), npo, b.mid, c.D(b1.d_off) + 2 * b1.C, c.D(b1.d_off) + 3 * b1.C, st));
        LCHK(run_bn_finalize(c, dw.bn, npo, 1));
      }
      bn_ss(b.cdw, &sc, &sf);
      float* pool = c.F(p.se_pool[bi]); float* sv = c.F(p.se[bi]); float* hpre = sv + (size_t)N * b.mid;
      LCHK(launch_swish_pool(c.F(p.y[b.cdw]), sc, sf, c.F(p.a1[bi]), N, (size_t)ho * wo, b.mid, pool, c.F(p.se_part), st));
      const ConvL& cr = m->convs[b.cr]; const ConvL& cx = m->convs[b.cx];
      LCHK(launch_se_fc_fwd(pool, m->params + cr.w_off, m->params + cr.bias_off, cr.Kpad, m->params + cx.w_off,
                            m->params + cx.bias_off, cx.Kpad, N, b.mid, b.nsq, hpre, hpre + (size_t)N * rup(b.nsq, 4), sv, st));
      LCHK(launch_se_scale(c.F(p.a1[bi]), sv, N, (size_t)ho * wo, b.mid, c.F(p.a2[bi]), st));
      Src a2 = mk_src(c.F(p.a2[bi]), b.mid, ho, wo);
      if (conv_bn(b.cp, a2, nullptr, ho, wo)) return 1;
      bn_ss(b.cp, &sc, &sf);
      const float* rs = (b.skip && b.drop > 0.f && m->keep_fwd) ? m->keep_fwd + bi * (size_t)N : nullptr;
      LCHK(launch_mb_out(c.F(p.y[b.cp]), sc, sf, rs, b.skip ? cur.ptr : nullptr, N, (size_t)ho * wo, b.Cout, c.F(p.xn[bi]), st));
      h = ho; w = wo;
      cur = mk_src(c.F(p.xn[bi]), b.Cout, h, w);
      for (int fs = 0; fs < 4; ++fs) if ((int)bi == m->feat_blk[fs]) feats[fs] = cur;
    }
  }
  Src d = feats[3];
  for (size_t i = 0; i < m->dec.size(); ++i) {
    const DecL& dl = m->dec[i];
    Src up = d; up.up = 1;
    h *= 2; w *= 2;
    Src skip; const Src* sp = nullptr;
    if (i < 3) { skip = feats[2 - i]; sp = &skip; }
    else if (i == 3) { skip = f1; sp = &skip; }
    if (sp && (skip.H != h || skip.W != w)) return fail("internal: skip shape mismatch at decoder block %d", (int)i);
    if (conv_bn(dl.c1, up, sp, h, w)) return 1;
    Src a1 = lazy_src(c, dl.c1, h, w);
    if (conv_bn(dl.c2, a1, nullptr, h, w)) return 1;
    d = lazy_src(c, dl.c2, h, w);
  }
  // UnetPlusPlus: dense grid of the same blocks; a node with several skip tensors gets them materialised (activation
  // applied) into one concat buffer, so every conv still sees two sources
  auto tensor_src = [&](int id) -> Src {
    if (id == 0) return f1;
    if (id < 5) return feats[id - 1];
    const NodeL& nd = m->nodes[id - 5];
    return lazy_src(c, nd.c2, H >> nd.lvl, W >> nd.lvl);
  };
  for (size_t i = 0; i < m->nodes.size(); ++i) {
    const NodeL& nd = m->nodes[i];
    h = H >> nd.lvl; w = W >> nd.lvl;
    Src up = tensor_src(nd.prev); up.up = 1;
    if (up.C != nd.C0 || (up.H << 1) != h || (up.W << 1) != w) return fail("internal: UnetPlusPlus node %d input mismatch", (int)i);
    Src skip; const Src* sp = nullptr;
    if (nd.skips.size() == 1) { skip = tensor_src(nd.skips[0]); sp = &skip; }
    else if (nd.skips.size() > 1) {
      int coff = 0;
      for (int id : nd.skips) {
        const Src t = tensor_src(id);
        if (t.H != h || t.W != w) return fail("internal: UnetPlusPlus node %d skip shape mismatch", (int)i);
        LCHK(launch_concat_copy(t, (size_t)N * h * w, c.F(p.cat[i]), nd.C1, coff, st));
        coff += t.C;
      }
      if (coff != nd.C1) return fail("internal: UnetPlusPlus node %d skip channels %d != %d", (int)i, coff, nd.C1);
      skip = mk_src(c.F(p.cat[i]), nd.C1, h, w); sp = &skip;
    }
    if (sp && (sp->C != nd.C1)) return fail("internal: UnetPlusPlus node %d skip channel mismatch", (int)i);
    if (conv_bn(nd.c1, up, sp, h, w)) return 1;
    Src a1 = lazy_src(c, nd.c1, h, w);
    if (conv_bn(nd.c2, a1, nullptr, h, w)) return 1;
    d = lazy_src(c, nd.c2, h, w);
  }
  (void)h1; (void)w1;
  LCHK(run_conv_fwd(c, m->head, d, nullptr, h, w, logits, false));
  return 0;
}
