// libuwm, part of uwm_model.hip (one translation unit; included from there): uwm_backward: staged backward (one gradient bucket per stage), weight gradients on the side stream.
// ------------------------------------------------------------------------------ backward
static int do_backward(uwm_model* m, const float* dlogits, float* ws, int sb, int se, hipStream_t st) {
  const Plan& p = m->plan;
  const int N = p.N, H = p.H, W = p.W;
  Ctx c{m, ws, st, N};
  c.wst = (m->use_side && m->side) ? m->side : st;
  // geometry
  const int h1 = H / 2, w1 = W / 2;          // f1
  int sh[4], sw[4];
  { int h = H / 4, w = W / 4; for (int s = 0; s < 4; ++s) { if (s > 0) { h /= 2; w /= 2; } sh[s] = h; sw[s] = w; } }
  std::vector<size_t> first_blk(4); { size_t b = 0; for (int s = 0; s < 4; ++s) { first_blk[s] = b; b += m->stages[s].size(); } }
  const bool effnet = !m->mb.empty();
  auto feat_blk = [&](int s) -> size_t { return effnet ? (size_t)m->feat_blk[s] : first_blk[s] + m->stages[s].size() - 1; };
  auto feat_src = [&](int s) {      // materialised output of encoder stage s (f2..f5)
    return mk_src(c.F(p.xn[feat_blk(s)]), m->featC[s], sh[s], sw[s]);
  };
  // ResNet features are ReLU outputs (the consumer's gradient is masked by feature > 0); EfficientNet's are linear
  auto feat_mask = [&](const Src& f) -> const float* { return effnet ? nullptr : f.ptr; };
  Src f1 = effnet ? mk_src(c.F(p.stem_a), m->f1C, h1, w1) : lazy_src(c, m->stem, h1, w1);

  std::vector<char>& out_sums = m->out_sums;
  if (sb <= 0 || out_sums.size() != first_blk[3] + m->stages[3].size()) out_sums.assign(first_blk[3] + m->stages[3].size(), 0);
  if (sb <= 0 || m->dy_max_made.size() != m->bns.size()) m->dy_max_made.assign(m->bns.size(), 0);     // (the slots are zeroed below)
  m->disp_cov.clear();
  if (sb <= 0) m->rq = ReduceQueue();                   // (a failed earlier call may have left jobs behind)
  if (sb <= 0 && se > 0) {
    HIPCHK(hipMemsetAsync(m->grads, 0, (size_t)m->param_floats * sizeof(float), st));
    // one memset for every BatchNorm's double scratch (the forward's sum/sumsq halves are dead after bn_finalize)
    HIPCHK(hipMemsetAsync(c.D(p.stat_d), 0, p.stat_d_count * sizeof(double), st));
    if (p.se_gs_floats) HIPCHK(hipMemsetAsync(c.F(p.se_gs_all), 0, p.se_gs_floats * sizeof(float), st));
    if (m->packed_in_fwd && m->pack_mode == pack_key(m)) {      // (a mode switch between forward and backward: redo them)
      HIPCHK(hipStreamWaitEvent(st, m->ev_pack, 0));
      m->packed_in_fwd = false;           // joined
    } else {
      if (m->packed_in_fwd) { HIPCHK(hipStreamWaitEvent(st, m->ev_pack, 0)); m->packed_in_fwd = false; }     // stale packs must have landed before they are overwritten
      for (size_t ci = 0; ci < m->convs.size(); ++ci) {
        const ConvL& cv = m->convs[ci];
        if (cv.dgrad && (!(cv.wud_off && p.wino_ok(ci)) || cv.CoutP == 16 || c16_f16_on(m, ci, true)))
          LCHK(launch_pack_dgrad(m->params + cv.w_off, cv.Cout, cv.Kpad, cv.k * cv.k, cv.CinP, c.F(cv.wd_off), cv.KpadD,
                                 cv.CoutP, st));
      }
      LCHK(wino_jobs(c, true, st));
    }
    // ---------------- head
    const ConvL& hd = m->convs[m->head];
    const int last_c2 = m->nodes.empty() ? m->dec.back().c2 : m->nodes.back().c2;
    Src d4 = lazy_src(c, last_c2, H, W);
    LCHK(run_wgrad(c, m->head, d4, nullptr, dlogits, H, W));
    LCHK(launch_colsum(dlogits, (size_t)N * H * W, hd.CoutP, m->grads + hd.bias_off, (double*)c.F(p.colsum_scr), st));
    bool head_sums = false;                               // BatchNorm-backward sums of the last decoder conv, made by the head's dgrad
    LCHK(run_dgrad(c, m->head, dlogits, H, W, H, W, c.F(p.g[last_c2]), nullptr, d4.ptr, d4.scale, d4.shift, nullptr,
                   m->convs[last_c2].bn, &head_sums));
    // ---------------- decoder blocks, last to first
    int h = H, w = W;
    bool c2_sums = head_sums;                              // BatchNorm-backward sums of dl.c2 already made by the dgrad that wrote its gradient
    for (int i = (int)m->dec.size() - 1; i >= 0; --i) {
      const DecL& dl = m->dec[i];
      const size_t npix = (size_t)N * h * w;
      LCHK(run_bn_bwd(c, dl.c2, c.F(p.g[dl.c2]), c.F(p.g[dl.c2]), npix, c2_sums));
      c2_sums = false;
      Src a1 = lazy_src(c, dl.c1, h, w);
      LCHK(run_wgrad(c, dl.c2, a1, nullptr, c.F(p.g[dl.c2]), h, w));
      bool c1_sums = false;
      LCHK(run_dgrad(c, dl.c2, c.F(p.g[dl.c2]), h, w, h, w, c.F(p.g[dl.c1]), nullptr, a1.ptr, a1.scale, a1.shift, nullptr,
                     m->convs[dl.c1].bn, &c1_sums));
      LCHK(run_bn_bwd(c, dl.c1, c.F(p.g[dl.c1]), c.F(p.g[dl.c1]), npix, c1_sums));
      // the block's input: cat(up(prev), skip)
      Src prev = (i == 0) ? feat_src(3) : lazy_src(c, m->dec[i - 1].c2, h / 2, w / 2);
      prev.up = 1;
      Src skip; const Src* sp = nullptr;
      if (i < 3) { skip = feat_src(2 - i); sp = &skip; } else if (i == 3) { skip = f1; sp = &skip; }
      LCHK(run_wgrad(c, dl.c1, prev, sp, c.F(p.g[dl.c1]), h, w));
      float* gprev = (i == 0) ? c.F(p.gx[feat_blk(3)]) : c.F(p.g[m->dec[i - 1].c2]);
      const float* pm = (i == 0) ? feat_mask(prev) : prev.ptr;
      const ConvL& c1v = m->convs[dl.c1];
      if (c1v.wud_off && p.wino_ok((size_t)dl.c1) && !(h & 1) && !(w & 1)) {
        // Winograd dgrad writes the 2x2-pooled, ReLU-masked gradient of up(prev) and the skip gradient directly:
        // the full-resolution dcat buffer and the upsplit pass never exist
        UpSplit us{gprev, dl.C0, pm, prev.scale, prev.shift, 0};
        // i > 0: gprev is the gradient wrt relu(bn(conv2 of block i-1)), masked by that conv's raw output: its BN sums ride along
        LCHK(run_dgrad(c, dl.c1, c.F(p.g[dl.c1]), h, w, h, w, dl.C1 > 0 ? c.F(p.gskip[i]) : nullptr, nullptr, nullptr, nullptr,
                       nullptr, &us, i > 0 ? m->convs[m->dec[i - 1].c2].bn : -1, &c2_sums));
      } else {
        LCHK(run_dgrad(c, dl.c1, c.F(p.g[dl.c1]), h, w, h, w, c.F(p.dcat[i]), nullptr, nullptr, nullptr, nullptr));
        LCHK(launch_upsplit(c.F(p.dcat[i]), N, h, w, dl.C0, dl.C1, gprev, pm, prev.scale, prev.shift,
                            dl.C1 > 0 ? c.F(p.gskip[i]) : nullptr, st));
      }
      h /= 2; w /= 2;
    }
    // ---------------- UnetPlusPlus nodes, last to first.  A tensor feeds several nodes: the first contribution to its
    // gradient buffer (in this order) writes, the others accumulate; ReLU masks are 0/1 factors, so masking each
    // contribution separately equals masking the sum.
    if (!m->nodes.empty()) {
      std::vector<char> ginit(5 + m->nodes.size(), 0);
      ginit[5 + m->nodes.size() - 1] = 1;                    // the head dgrad wrote the last node's gradient
      auto tensor_src = [&](int id) -> Src {
        if (id == 0) return f1;
        if (id < 5) return feat_src(id - 1);
        const NodeL& nd = m->nodes[id - 5];
        return lazy_src(c, nd.c2, H >> nd.lvl, W >> nd.lvl);
      };
      auto tensor_grad = [&](int id) -> float* {             // f1..f4 -> gskip[3..0], f5 -> gx of the last encoder block
        if (id < 4) return c.F(p.gskip[3 - id]);
        if (id == 4) return c.F(p.gx[feat_blk(3)]);
        return c.F(p.g[m->nodes[id - 5].c2]);
      };
      for (int i = (int)m->nodes.size() - 1; i >= 0; --i) {
        const NodeL& nd = m->nodes[i];
        const int nh = H >> nd.lvl, nw = W >> nd.lvl;
        const size_t npix = (size_t)N * nh * nw;
        if (!ginit[5 + i]) return fail("internal: UnetPlusPlus node %d has no consumer", i);
        LCHK(run_bn_bwd(c, nd.c2, c.F(p.g[nd.c2]), c.F(p.g[nd.c2]), npix, i == (int)m->nodes.size() - 1 && head_sums));
        Src a1 = lazy_src(c, nd.c1, nh, nw);
        LCHK(run_wgrad(c, nd.c2, a1, nullptr, c.F(p.g[nd.c2]), nh, nw));
        bool c1_sums = false;
        LCHK(run_dgrad(c, nd.c2, c.F(p.g[nd.c2]), nh, nw, nh, nw, c.F(p.g[nd.c1]), nullptr, a1.ptr, a1.scale, a1.shift, nullptr,
                       m->convs[nd.c1].bn, &c1_sums));
        LCHK(run_bn_bwd(c, nd.c1, c.F(p.g[nd.c1]), c.F(p.g[nd.c1]), npix, c1_sums));
        Src prev = tensor_src(nd.prev); prev.up = 1;
        Src skip; const Src* sp = nullptr;
        if (nd.skips.size() == 1) { skip = tensor_src(nd.skips[0]); sp = &skip; }
        else if (nd.skips.size() > 1) { skip = mk_src(c.F(p.cat[i]), nd.C1, nh, nw); sp = &skip; }
        LCHK(run_wgrad(c, nd.c1, prev, sp, c.F(p.g[nd.c1]), nh, nw));
        float* gprev = tensor_grad(nd.prev);
        const float* pm = nd.prev < 5 ? feat_mask(prev) : prev.ptr;
        const int acc_prev = ginit[nd.prev]; ginit[nd.prev] = 1;
        const ConvL& c1v = m->convs[nd.c1];
        const float* gcat; int gcc, gco;                      // where the skip part of the gradient lands
        if (c1v.wud_off && p.wino_ok((size_t)nd.c1) && !(nh & 1) && !(nw & 1)) {
          UpSplit us{gprev, nd.C0, pm, prev.scale, prev.shift, acc_prev};
          LCHK(run_dgrad(c, nd.c1, c.F(p.g[nd.c1]), nh, nw, nh, nw, nd.C1 > 0 ? c.F(p.gcat) : nullptr, nullptr, nullptr, nullptr,
                         nullptr, &us));
          gcat = c.F(p.gcat); gcc = nd.C1; gco = 0;
        } else {
          LCHK(run_dgrad(c, nd.c1, c.F(p.g[nd.c1]), nh, nw, nh, nw, c.F(p.dcat[0]), nullptr, nullptr, nullptr, nullptr));
          LCHK(launch_upsplit(c.F(p.dcat[0]), N, nh, nw, nd.C0, nd.C1, gprev, pm, prev.scale, prev.shift, nullptr, st, acc_prev));
          gcat = c.F(p.dcat[0]); gcc = nd.C0 + nd.C1; gco = nd.C0;
        }
        int coff = 0;
        for (int id : nd.skips) {
          const Src t = tensor_src(id);
          const bool lazy_mask = id >= 5;                     // node outputs: mask by their own ReLU; encoder features: the encoder masks
          LCHK(launch_split_accum(gcat, gcc, gco + coff, t.C, npix, tensor_grad(id), lazy_mask ? t.ptr : nullptr,
                                  lazy_mask ? t.scale : nullptr, lazy_mask ? t.shift : nullptr, ginit[id], st));
          ginit[id] = 1;
          coff += t.C;
        }
      }
      for (int id = 0; id < 5; ++id) if (!ginit[id]) return fail("internal: UnetPlusPlus feature %d received no gradient", id);
    }
  }
  // ---------------- EfficientNet encoder: backward stage k handles the blocks between features f_{5-k} and f_{6-k}
  for (int k = (sb < 1 ? 1 : sb); effnet && k < se && k <= 4; ++k) {
    const int s = 4 - k;
    const int lo = s == 0 ? 0 : m->feat_blk[s - 1] + 1;
    for (int bi = m->feat_blk[s]; bi >= lo; --bi) {
      const MBL& b = m->mb[bi];
      const int ho = p.mh[bi], wo = p.mw[bi], hi = ho * b.stride, wi = wo * b.stride;
      const size_t npo = (size_t)N * ho * wo, npi = (size_t)N * hi * wi;
      const float* dz = c.F(p.gx[bi]);                       // grad wrt the block output (complete)
      float* gO = c.F(p.g[b.cp]); float* gM = c.F(p.g[b.cdw]);
      const float* rs = (b.skip && b.drop > 0.f && m->keep_fwd) ? m->keep_fwd + (size_t)bi * N : nullptr;
      const float* g2 = dz;
      if (rs) { LCHK(launch_rowscale(dz, rs, N, (size_t)ho * wo, b.Cout, gO, st)); g2 = gO; }
      LCHK(run_bn_bwd(c, b.cp, g2, gO, npo));
      Src a2 = mk_src(c.F(p.a2[bi]), b.mid, ho, wo);
      LCHK(run_wgrad(c, b.cp, a2, nullptr, gO, ho, wo));
      LCHK(run_dgrad(c, b.cp, gO, ho, wo, ho, wo, gM, nullptr, nullptr, nullptr, nullptr));
      // squeeze-and-excitation: gs = sum_hw g*a1 ; FC backward ; g_a1 = g*s + gpool/hw, then through swish(bn1(.))
      float* pool = c.F(p.se_pool[bi]); float* sv = c.F(p.se[bi]); float* hpre = sv + (size_t)N * b.mid;
      float* gs = c.F(p.se_gs[bi]); float* acc1 = gs + (size_t)N * b.mid; float* gpool = c.F(p.se_g);      // gs / acc1 zeroed at the start of the backward
      LCHK(launch_se_reduce_hw(gM, c.F(p.a1[bi]), N, (size_t)ho * wo, b.mid, 1.f, gs, c.F(p.se_part), st));
      const ConvL& cr = m->convs[b.cr]; const ConvL& cx = m->convs[b.cx];
      LCHK(launch_se_fc_bwd(gs, sv, hpre, pool, m->params + cr.w_off, cr.Kpad, m->params + cx.w_off, cx.Kpad, N, b.mid, b.nsq,
                            gpool, acc1, m->grads + cr.w_off, m->grads + cr.bias_off, m->grads + cx.w_off, m->grads + cx.bias_off, st));
      LCHK(run_bn_bwd_act(c, b.cdw, gM, gM, N, (size_t)ho * wo, sv, gpool));
      // block input and where its gradient goes
      Src in = bi == 0 ? f1 : mk_src(c.F(p.xn[bi - 1]), b.Cin, hi, wi);
      float* gin = bi == 0 ? c.F(p.g[m->stem]) : c.F(p.gx[bi - 1]);
      const float* addend = nullptr;
      if (b.skip) addend = dz;                                // identity shortcut
      else if (bi == 0) addend = c.F(p.gskip[3]);             // f1's gradient from the decoder
      else for (int fs = 0; fs < 3; ++fs) if (bi - 1 == m->feat_blk[fs]) addend = c.F(p.gskip[2 - fs]);   // f2..f4
      const ConvL& dw = m->convs[b.cdw];
      const float* dwin = b.ce >= 0 ? c.F(p.a0[bi]) : in.ptr;
      {
        hipStream_t ws_ = st;
        if (c.wst && c.wst != st) { HIPCHK(hipEventRecord(m->ev_fork, st)); HIPCHK(hipStreamWaitEvent(c.wst, m->ev_fork, 0)); ws_ = c.wst; }
        LCHK(launch_dw_wgrad(dwin, gM, b.k, b.stride, b.pb, N, hi, wi, b.mid, ho, wo, m->grads + dw.w_off, c.F(p.dw_part), ws_));
      }
      if (b.ce >= 0) {
        float* gI = c.F(p.g[b.ce]);
        LCHK(launch_dw_dgrad(gM, m->params + dw.w_off, b.k, b.stride, b.pb, N, hi, wi, b.mid, ho, wo, nullptr, gI, st));
        LCHK(run_bn_bwd_act(c, b.ce, gI, gI, N, (size_t)hi * wi, nullptr, nullptr));
        LCHK(run_wgrad(c, b.ce, in, nullptr, gI, hi, wi));
        LCHK(run_dgrad(c, b.ce, gI, hi, wi, hi, wi, gin, addend, nullptr, nullptr, nullptr));
      } else {
        LCHK(launch_dw_dgrad(gM, m->params + dw.w_off, b.k, b.stride, b.pb, N, hi, wi, b.mid, ho, wo, addend, gin, st));
      }
    }
    if (s == 0) {
      float* g = c.F(p.g[m->stem]);
      LCHK(run_bn_bwd_act(c, m->stem, g, g, N, (size_t)h1 * w1, nullptr, nullptr));
      Src x4 = mk_src(c.F(p.x4), m->CinP, H, W);
      LCHK(run_wgrad(c, m->stem, x4, nullptr, g, h1, w1));
    }
  }
  // ---------------- encoder stages: backward stage k handles encoder stage s = 4 - k
  for (int k = (sb < 1 ? 1 : sb); !effnet && k < se && k <= 4; ++k) {
    const int s = 4 - k;
    const int h = sh[s], w = sw[s];
    const size_t npix = (size_t)N * h * w;
    for (int b = (int)m->stages[s].size() - 1; b >= 0; --b) {
      const BlockL& bl = m->stages[s][b];
      const size_t bi = first_blk[s] + b;
      const float* dz = c.F(p.gx[bi]);                       // masked grad wrt the block output
      const int lc = bl.last();
      const int hin = h * bl.stride, win = w * bl.stride;
      LCHK(run_bn_bwd(c, lc, dz, c.F(p.g[lc]), npix, out_sums[bi] != 0));
      if (bl.cd >= 0) LCHK(run_bn_bwd(c, bl.cd, dz, c.F(p.g[bl.cd]), npix));
      int hc1 = h, wc1 = w;                                  // resolution of c1's output
      if (bl.c3 >= 0) {                                      // Bottleneck tail: conv3 (1x1) <- relu(bn2(conv2))
        Src a2 = lazy_src(c, bl.c2, h, w);
        LCHK(run_wgrad(c, bl.c3, a2, nullptr, c.F(p.g[bl.c3]), h, w));
        bool c2_sums = false;                                // conv3's 1x1 dgrad (implicit GEMM epilogue) carries bn2's backward sums
        LCHK(run_dgrad(c, bl.c3, c.F(p.g[bl.c3]), h, w, h, w, c.F(p.g[bl.c2]), nullptr, a2.ptr, a2.scale, a2.shift, nullptr,
                       m->convs[bl.c2].bn, &c2_sums));
        LCHK(run_bn_bwd(c, bl.c2, c.F(p.g[bl.c2]), c.F(p.g[bl.c2]), npix, c2_sums));
        hc1 = hin; wc1 = win;
      }
      Src a1 = lazy_src(c, bl.c1, hc1, wc1);
      LCHK(run_wgrad(c, bl.c2, a1, nullptr, c.F(p.g[bl.c2]), h, w));
      bool c1_sums = false;
      LCHK(run_dgrad(c, bl.c2, c.F(p.g[bl.c2]), h, w, hc1, wc1, c.F(p.g[bl.c1]), nullptr, a1.ptr, a1.scale, a1.shift, nullptr,
                     m->convs[bl.c1].bn, &c1_sums));
      LCHK(run_bn_bwd(c, bl.c1, c.F(p.g[bl.c1]), c.F(p.g[bl.c1]), (size_t)N * hc1 * wc1, c1_sums));
      // block input
      Src in; float* gin; const float* in_mask;
      if (b > 0) { in = mk_src(c.F(p.xn[bi - 1]), bl.Cin, hin, win); gin = c.F(p.gx[bi - 1]); in_mask = in.ptr; }
      else if (s > 0) { in = feat_src(s - 1); gin = c.F(p.gx[first_blk[s] - 1]); in_mask = in.ptr; }
      else { in = mk_src(c.F(p.pool), 64, hin, win); gin = c.F(p.g_pool); in_mask = nullptr; }
      LCHK(run_wgrad(c, bl.c1, in, nullptr, c.F(p.g[bl.c1]), hc1, wc1));
      const float* addend;
      if (bl.cd >= 0) {
        LCHK(run_wgrad(c, bl.cd, in, nullptr, c.F(p.g[bl.cd]), h, w));
        // skip-connection gradient from the decoder for this feature (f2,f3,f4 <- dec blocks 2,1,0)
        const float* gs = (b == 0 && s > 0) ? c.F(p.gskip[3 - s]) : nullptr;
        LCHK(run_dgrad(c, bl.cd, c.F(p.g[bl.cd]), h, w, hin, win, c.F(p.tmp), gs, nullptr, nullptr, nullptr));
        addend = c.F(p.tmp);
      } else {
        addend = dz;                                         // identity shortcut
      }
      // gin is the (masked) gradient wrt the PREVIOUS block's output = the gradient wrt that block's last BatchNorm output: its
      // backward sums ride in this epilogue, yhat read from that BatchNorm's raw input (run_dgrad bn_y)
      int pbn = -1; const float* py = nullptr; size_t pbi = 0;
      if (b > 0) { pbi = bi - 1; const int plc = m->stages[s][b - 1].last(); pbn = m->convs[plc].bn; py = c.F(p.y[plc]); }
      else if (s > 0) { pbi = first_blk[s] - 1; const int plc = m->stages[s - 1].back().last(); pbn = m->convs[plc].bn; py = c.F(p.y[plc]); }
      bool psums = false;
      LCHK(run_dgrad(c, bl.c1, c.F(p.g[bl.c1]), hc1, wc1, hin, win, gin, addend, in_mask, nullptr, nullptr, nullptr, pbn, &psums, py));
      if (pbn >= 0) out_sums[pbi] = psums ? 1 : 0;
    }
    if (s == 0) {
      // maxpool backward (+ decoder skip gradient for f1) -> stem BN backward -> stem wgrad
      // the masked gradient it writes is the gradient wrt the stem BatchNorm's output and it reads that BatchNorm's raw input
      // for the mask anyway: the BatchNorm-backward sums ride along (replicas of the forward statistics, re-zeroed above)
      const BNL& sb = m->bns[m->convs[m->stem].bn];
      static const bool no_fuse = dbg_flag("UWM_NO_BN_FUSE");
      const bool pool_sums = !no_fuse && f1.scale && f1.relu && sb.C == f1.C && (256 % (f1.C / 4)) == 0;
      // the queued partial-sum reduces of this stage go NOW, behind layer1's weight gradients and beside the max-pool / BatchNorm
      // backward: the stem's weight gradient (its own reduce) is then all that is left between the last dgrad-chain kernel and Adam
      LCHK(launch_wgrad_reduce_multi(m->rq, c.wst));
      LCHK(launch_maxpool_bwd(c.F(p.g_pool), (const uint8_t*)c.F(p.pool_idx), c.F(p.gskip[3]), f1, c.F(p.g[m->stem]), N,
                              sh[0], sw[0], st, pool_sums ? c.F(sb.f_off) : nullptr, pool_sums ? c.F(sb.f_off) + sb.C : nullptr,
                              c.D(sb.d_off) + 2 * sb.C, c.D(sb.d_off) + 3 * sb.C, sb.nrep, 2 * sb.C));
      LCHK(run_bn_bwd(c, m->stem, c.F(p.g[m->stem]), c.F(p.g[m->stem]), (size_t)N * h1 * w1, pool_sums));
      Src x4 = mk_src(c.F(p.x4), m->CinP, H, W);
      LCHK(run_wgrad(c, m->stem, x4, nullptr, c.F(p.g[m->stem]), h1, w1));
    }
  }
  LCHK(launch_wgrad_reduce_multi(m->rq, c.wst));      // the queued partial-sum reduces of these stages: one launch
  if (c.wst != st) {                    // join: the caller's stream waits for every wgrad of these stages
    HIPCHK(hipEventRecord(m->ev_join, c.wst));
    // data-parallel training hands in its communication stream: the bucket's all-reduce waits for this stage's weight
    // gradients, the caller's stream runs on into the next stage's dgrad chain (nothing there reads what the side
    // stream still writes).  The LAST stage always joins the caller's stream: the optimizer comes next.
    HIPCHK(hipStreamWaitEvent((m->join_stream && se < 5) ? m->join_stream : st, m->ev_join, 0));
    if (m->join_stream && se >= 5) HIPCHK(hipStreamWaitEvent(m->join_stream, m->ev_join, 0));
  }
  return 0;
}
