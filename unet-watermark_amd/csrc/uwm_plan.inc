// libuwm, part of uwm_model.hip (one translation unit; included from there): workspace plan of one (N, H, W, training) and the per-layer routing predicates (which kernel family a layer takes under the handle's Winograd / precision modes).
// ------------------------------------------------------------------------------ workspace plan
static void make_plan(uwm_model* m, int N, int H, int W, int training) {
  Plan p; p.N = N; p.H = H; p.W = W; p.training = training; p.wino_mode = m->wino_mode; p.prec = m->prec;
  size_t off = m->fixed_floats;
  auto alloc = [&](size_t floats) { size_t o = off; off += (size_t)rup((long long)floats, 64); return o; };
  const size_t nc = m->convs.size();
  p.y.assign(nc, 0); p.g.assign(nc, 0); p.oh.assign(nc, 0); p.ow.assign(nc, 0);
  p.stat_d = 0; p.stat_d_count = 0; for (auto& b : m->bns) p.stat_d_count += b.dcount();
  p.loss_scr = alloc(64);
  p.x4 = alloc((size_t)N * H * W * m->CinP);
  int h = H / 2, w = W / 2;
  const int stemC = m->convs[m->stem].CoutP;
  p.y[m->stem] = alloc((size_t)N * h * w * stemC); p.oh[m->stem] = h; p.ow[m->stem] = w;
  size_t nblk = m->mb.size(); for (auto& s : m->stages) nblk += s.size();
  p.xn.assign(nblk, 0); p.gx.assign(nblk, 0);
  size_t bi = 0; size_t max_in = 0, max_mid = 0, max_nsq = 0;
  auto place = [&](int ci, int oh, int ow) { p.y[ci] = alloc((size_t)N * oh * ow * m->convs[ci].CoutP); p.oh[ci] = oh; p.ow[ci] = ow; };
  if (m->mb.empty()) {
    h /= 2; w /= 2;
    p.pool = alloc((size_t)N * h * w * 64);
    p.pool_idx = alloc((size_t)N * h * w * 64 / 4 + 64);
    max_in = (size_t)N * h * w * 64;
    for (int s = 0; s < 4; ++s) {
      for (auto& bl : m->stages[s]) {
        const int hi = h, wi = w;
        h /= bl.stride; w /= bl.stride;
        if (bl.c3 < 0) { place(bl.c1, h, w); place(bl.c2, h, w); }
        else { place(bl.c1, hi, wi); place(bl.c2, h, w); place(bl.c3, h, w); }
        if (bl.cd >= 0) place(bl.cd, h, w);
        const size_t sz = (size_t)N * h * w * bl.Cout;
        p.xn[bi++] = alloc(sz);
        if (sz > max_in) max_in = sz;
        if ((size_t)N * hi * wi * bl.Cin > max_in) max_in = (size_t)N * hi * wi * bl.Cin;
      }
    }
  } else {
    p.stem_a = alloc((size_t)N * h * w * stemC);
    const size_t nb = m->mb.size();
    p.a0.assign(nb, 0); p.a1.assign(nb, 0); p.a2.assign(nb, 0); p.se.assign(nb, 0); p.mh.assign(nb, 0); p.mw.assign(nb, 0);
    p.se_pool.assign(nb, 0); p.se_gs.assign(nb, 0);
    for (size_t i = 0; i < nb; ++i) { p.se_pool[i] = p.se_pool_floats; p.se_pool_floats += (size_t)rup((long long)N * m->mb[i].mid, 64); }
    p.se_pool_all = alloc(p.se_pool_floats);
    { size_t mm = 0; for (auto& b : m->mb) mm = std::max(mm, (size_t)b.mid); p.se_part = alloc(se_reduce_scratch_floats(N, (int)mm)); }
    for (size_t i = 0; i < nb; ++i) p.se_pool[i] += p.se_pool_all;
    for (; bi < nb; ++bi) {
      const MBL& b = m->mb[bi];
      const int hi = h, wi = w;
      h /= b.stride; w /= b.stride;
      if (b.ce >= 0) { place(b.ce, hi, wi); p.a0[bi] = alloc((size_t)N * hi * wi * b.mid); }
      place(b.cdw, h, w);
      p.a1[bi] = alloc((size_t)N * h * w * b.mid); p.a2[bi] = alloc((size_t)N * h * w * b.mid);
      p.se[bi] = alloc((size_t)N * (b.mid + 2 * (size_t)rup(b.nsq, 4)));        // {s [N][mid], hpre [N][nsq], hid [N][nsq]}
      place(b.cp, h, w);
      p.oh[b.cr] = p.ow[b.cr] = p.oh[b.cx] = p.ow[b.cx] = 1;
      p.xn[bi] = alloc((size_t)N * h * w * b.Cout);
      p.mh[bi] = h; p.mw[bi] = w;
      max_mid = std::max(max_mid, (size_t)b.mid); max_nsq = std::max(max_nsq, (size_t)rup(b.nsq, 4));
    }
  }
  for (size_t i = 0; i < m->dec.size(); ++i) {
    h *= 2; w *= 2;
    const size_t sz = (size_t)N * h * w * m->convs[m->dec[i].c1].Cout;
    p.y[m->dec[i].c1] = alloc(sz); p.y[m->dec[i].c2] = alloc(sz);
    p.oh[m->dec[i].c1] = p.oh[m->dec[i].c2] = h; p.ow[m->dec[i].c1] = p.ow[m->dec[i].c2] = w;
  }
  p.cat.assign(m->nodes.size(), 0);
  size_t max_gcat = 0, max_dcat = 0;
  for (size_t i = 0; i < m->nodes.size(); ++i) {
    const NodeL& nd = m->nodes[i];
    const int nh = H >> nd.lvl, nw = W >> nd.lvl;
    const size_t sz = (size_t)N * nh * nw * m->convs[nd.c1].Cout;
    p.y[nd.c1] = alloc(sz); p.y[nd.c2] = alloc(sz);
    p.oh[nd.c1] = p.oh[nd.c2] = nh; p.ow[nd.c1] = p.ow[nd.c2] = nw;
    if (nd.skips.size() > 1) p.cat[i] = alloc((size_t)N * nh * nw * nd.C1);
    max_gcat = std::max(max_gcat, (size_t)N * nh * nw * nd.C1);
    max_dcat = std::max(max_dcat, (size_t)N * nh * nw * (nd.C0 + nd.C1));
  }
  p.oh[m->head] = H; p.ow[m->head] = W;
  if (training) {
    p.colsum_scr = alloc(2 * colsum_scratch_doubles(m->CP));
    p.wg_part = alloc(kWgParts * wgrad_wino_scratch_floats());      // several layers' partial images wait for one batched reduce
    // gradient buffers (same shapes as their activations)
    h = H / 2; w = W / 2;
    p.g[m->stem] = alloc((size_t)N * h * w * stemC);
    if (m->mb.empty()) {
      h /= 2; w /= 2;
      p.g_pool = alloc((size_t)N * h * w * 64);
      bi = 0;
      for (int s = 0; s < 4; ++s)
        for (auto& bl : m->stages[s]) {
          for (int ci : {bl.c1, bl.c2, bl.c3, bl.cd})
            if (ci >= 0) p.g[ci] = alloc((size_t)N * p.oh[ci] * p.ow[ci] * m->convs[ci].Cout);
          p.gx[bi++] = alloc((size_t)N * p.oh[bl.c2] * p.ow[bl.c2] * bl.Cout);
        }
      p.tmp = alloc(max_in);
    } else {
      for (size_t i = 0; i < m->mb.size(); ++i) {
        const MBL& b = m->mb[i];
        for (int ci : {b.ce, b.cdw, b.cp})
          if (ci >= 0) p.g[ci] = alloc((size_t)N * p.oh[ci] * p.ow[ci] * m->convs[ci].CoutP);
        p.gx[i] = alloc((size_t)N * p.mh[i] * p.mw[i] * b.Cout);
      }
      size_t max_part = 0;
      for (size_t i = 0; i < m->mb.size(); ++i) max_part = std::max(max_part, dw_wgrad_scratch_floats(m->mb[i].k, N, m->mb[i].mid, p.mh[i], p.mw[i]));
      p.dw_part = alloc(max_part);
      p.se_g = alloc((size_t)N * max_mid);
      for (size_t i = 0; i < m->mb.size(); ++i) { p.se_gs[i] = p.se_gs_floats; p.se_gs_floats += (size_t)rup((long long)N * (m->mb[i].mid + m->mb[i].nsq), 64); }
      p.se_gs_all = alloc(p.se_gs_floats);
      for (size_t i = 0; i < m->mb.size(); ++i) p.se_gs[i] += p.se_gs_all;
    }
    h = H / 32; w = W / 32;                       // deepest feature: the decoder loop below doubles from here
    p.dcat.assign(m->dec.size(), 0); p.gskip.assign(m->dec.size(), 0);
    for (size_t i = 0; i < m->dec.size(); ++i) {
      h *= 2; w *= 2;
      const DecL& d = m->dec[i];
      const size_t sz = (size_t)N * h * w * m->convs[d.c1].Cout;
      p.g[d.c1] = alloc(sz); p.g[d.c2] = alloc(sz);
      p.dcat[i] = alloc((size_t)N * h * w * (d.C0 + d.C1));
      if (d.C1 > 0) p.gskip[i] = alloc((size_t)N * h * w * d.C1);
    }
    if (!m->nodes.empty()) {
      for (auto& nd : m->nodes) {
        const size_t sz = (size_t)N * (H >> nd.lvl) * (W >> nd.lvl) * m->convs[nd.c1].Cout;
        p.g[nd.c1] = alloc(sz); p.g[nd.c2] = alloc(sz);
      }
      p.dcat.assign(1, alloc(max_dcat));
      p.gcat = alloc(max_gcat);
      const int fc[4] = {m->featC[2], m->featC[1], m->featC[0], m->f1C};       // gradient accumulators of f4, f3, f2, f1
      p.gskip.assign(4, 0);
      for (int j = 0; j < 4; ++j) p.gskip[j] = alloc((size_t)N * (H >> (4 - j)) * (W >> (4 - j)) * fc[j]);
    }
  }
  p.bytes = off * sizeof(float);
  m->plan = p;
}

// The fill rule of the fp16x3 kernels: the launch gives at least every second CU a workgroup (uwm_set_precision_fill: another bar; uwm_set_routing_batch: another batch)
static bool fills_chip(const uwm_model* m, long wgs_per_image, int per_cu = 1) {
  const long wgs = (long)(m->route_n > 0 ? m->route_n : m->plan.N) * wgs_per_image;
  return wgs >= (long)(m->f3_min_wgs > 0 ? m->f3_min_wgs : device_cu_count() / 2) * per_cu;
}
// conv ci as the conv1 of decoder block `block` (m->dec / m->nodes; -1: it is none): its input = concat(upsampled tensor: C0 channels, skips: C1)
struct Conv1 { int block, C0, C1; };
static Conv1 conv1_of(const uwm_model* m, size_t ci) {
  for (size_t i = 0; i < m->dec.size(); ++i) if (m->dec[i].c1 == (int)ci) return {(int)i, m->dec[i].C0, m->dec[i].C1};
  for (size_t i = 0; i < m->nodes.size(); ++i) if (m->nodes[i].c1 == (int)ci) return {(int)i, m->nodes[i].C0, m->nodes[i].C1};
  return {-1, 0, 0};
}
// decoder block 4 conv2 (3x3, 16 -> 16 at full resolution) and block 3 conv2 (32 -> 32) on conv_c16_f16.hip, forward (fp16x3 modes) and dgrad (f16x3_all modes):
// whole 8 x 32 tiles, the same fill rule as the other fp16x3 kernels
static bool c16_f16_on(const uwm_model* m, size_t ci, bool dgrad) {
  const ConvL& cv = m->convs[ci]; const Plan& p = m->plan;
  static const bool off = dbg_flag("UWM_NO_C16_F16");
  static const bool off32 = dbg_flag("UWM_NO_C32_F16");
  const bool c16 = cv.CinP == 16 && cv.c0 == 16 && cv.CoutP == 16 && cv.Cout == 16;
  const bool c32 = !off32 && cv.CinP == 32 && cv.c0 == 32 && cv.CoutP == 32 && cv.Cout == 32;      // decoder block 3 conv2: conv_c32_f16_kernel
  if (off || cv.bn < 0 || cv.dw || cv.k != 3 || cv.stride != 1 || cv.pad != 1 || !(c16 || c32)) return false;
  if (p.prec < (dgrad ? UWM_PREC_F16X3_ALL : UWM_PREC_F16X3) || (dgrad && !cv.dgrad) || p.wino_mode == 0) return false;
  if ((p.oh[ci] % 8) || (p.ow[ci] % 32)) return false;
  return fills_chip(m, (long)(p.oh[ci] / 8) * (p.ow[ci] / 32), c32 ? 2 : 1);      // (32 channels: ONE workgroup per CU walks the tiles)
}
// a conv takes the fp16x3 direct kernel (forward) when its shape is eligible AND the launch fills the chip: 16x16-pixel x 64-channel
// workgroups, at least one per two CUs (measured: 973 vs 952 img/s with layer4's 128-workgroup launches on it; smaller launches
// — small batch / resolution — stay on the Winograd kernels)
static bool f3_fwd_on(const uwm_model* m, size_t ci) {
  const ConvL& cv = m->convs[ci]; const Plan& p = m->plan;
  if (p.prec < UWM_PREC_F16X3 || !cv.f3() || !p.wino_ok(ci) || c16_f16_on(m, ci, false)) return false;
  return fills_chip(m, (long)((p.oh[ci] + 15) / 16) * ((p.ow[ci] + 15) / 16) * ((cv.Cout + 63) / 64));
}
// the stem on conv_stem_f16x3: fp16x3 forward modes, the same fill rule over its 16x16-pixel workgroups
static bool stem_f3_on(const uwm_model* m) {
  if (m->stem < 0) return false;
  const ConvL& cv = m->convs[m->stem]; const Plan& p = m->plan;
  if (p.prec < UWM_PREC_F16X3 || !cv.stem7() || !cv.wu_off || p.wino_mode == 0 || dbg_flag("UWM_NO_STEM_F16X3")) return false;
  return fills_chip(m, (long)((p.oh[m->stem] + 15) / 16) * ((p.ow[m->stem] + 15) / 16));
}
// a decoder conv1's dgrad splits the concat gradient in its epilogue (ConvArgs::out_up): the fp16x3 kernel takes it when the
// boundary sits on a 64-channel tile
static bool f3d_plain(const uwm_model* m, size_t ci) { return (conv1_of(m, ci).C0 & 63) == 0; }      // (no conv1: C0 = 0)
// fp16x3 weight gradient: the map tiled by whole 4 x 32- or 8 x 16-pixel stages, 32-channel tiles on either side of the concat
static bool f3_wgrad_on(const uwm_model* m, size_t ci) {
  const ConvL& cv = m->convs[ci]; const Plan& p = m->plan;
  return p.prec >= UWM_PREC_F16X3_ALL && cv.wino() && cv.bn >= 0 && cv.Cout >= 32 && (cv.CinP & 31) == 0 && (cv.c0 & 31) == 0 && cv.Kpad == 9 * cv.CinP &&
         (((p.ow[ci] % 32) == 0 && (p.oh[ci] % 4) == 0) || ((p.ow[ci] % 16) == 0 && (p.oh[ci] % 8) == 0)) && !dbg_flag("UWM_NO_F16X3_WGRAD");
}
static bool f3_dgrad_on(const uwm_model* m, size_t ci) {
  const ConvL& cv = m->convs[ci]; const Plan& p = m->plan;
  if (p.prec < UWM_PREC_F16X3_ALL || !cv.f3_d() || cv.bn < 0 || !p.wino_ok(ci) || !f3d_plain(m, ci) || c16_f16_on(m, ci, true)) return false;
  return fills_chip(m, (long)((p.oh[ci] + 15) / 16) * ((p.ow[ci] + 15) / 16) * ((cv.CinP + 63) / 64));      // (stride 1: the input has the output's size)
}
// stride-2 layers of the ResNet encoders (3x3 / stride 2 and the 1x1 / stride 2 downsample) and the 1x1 / stride-1 layers of the
// Bottleneck encoders on the implicit GEMM / the 1x1 GEMM with fp16x3
// split products (ConvArgs::ig16) in the fp16x3 modes: forward from UWM_PREC_F16X3 on, their dgrads from UWM_PREC_F16X3_ALL on
static bool ig16_on(const uwm_model* m, size_t ci, bool dgrad) {
  const ConvL& cv = m->convs[ci]; const int pm = m->plan.prec;
  static const bool off = dbg_flag("UWM_NO_IG16");
  static const bool off11 = dbg_flag("UWM_NO_IG16_1X1");
  const bool s2 = cv.stride == 2 && (cv.k == 3 || cv.k == 1);
  const bool p11 = !off11 && cv.stride == 1 && cv.k == 1 && cv.pad == 0;      // round 4: the 1x1 / stride-1 layers (Bottleneck conv1 / conv3 / layer1's downsample: conv_gemm.hip's F16 form)
  if (off || cv.dw || cv.bn < 0 || !(s2 || p11) || (cv.CinP & 31) || (cv.CoutP & 31)) return false;
  return dgrad ? (pm >= UWM_PREC_F16X3_ALL && cv.dgrad) : pm >= UWM_PREC_F16X3;
}
// ... with the weight operand pre-split into a bank (ConvL::igb, wino_jobs; UWM_NO_IG_BANK: split while staging, as before)
static bool ig_bank_on(const uwm_model* m, size_t ci, bool dgrad) {
  static const bool off = dbg_flag("UWM_NO_IG_BANK");
  const ConvL& cv = m->convs[ci];
  return !off && cv.igb() && (dgrad ? cv.wdb_off : cv.wu_off) != 0 && ig16_on(m, ci, dgrad);
}
// the sub-pixel decoder conv (3x3 over the x2-upsampled 32-channel map, 16 outputs, no skip: conv_up2.hip) on conv_up2_f16.hip's
// fp16x3 kernels: forward from UWM_PREC_F16X3 on, its dgrad from UWM_PREC_F16X3_ALL on
static bool up2_f16_on(const uwm_model* m, size_t ci, bool dgrad) {
  const ConvL& cv = m->convs[ci]; const int pm = m->plan.prec;
  static const bool off = dbg_flag("UWM_NO_UP2_F16");
  if (off || cv.bn < 0 || cv.k != 3 || cv.stride != 1 || cv.CinP != 32 || cv.CoutP != 16) return false;
  const Conv1 c1 = conv1_of(m, ci);
  if (c1.block < 0 || c1.C1 != 0) return false;
  return dgrad ? pm >= UWM_PREC_F16X3_ALL : pm >= UWM_PREC_F16X3;
}
// the ResNet stem's weight gradient on wgrad_stem.hip's fp16x3 kernel (the last kernel of the step): from UWM_PREC_F16X3_ALL on
static bool stem_wg16_on(const uwm_model* m, size_t ci) {
  static const bool off = dbg_flag("UWM_NO_STEM_WG16");
  return !off && (int)ci == m->stem && m->plan.prec >= UWM_PREC_F16X3_ALL && m->convs[ci].stem7() && m->convs[ci].bn >= 0;
}
// the 16 -> 16 full-resolution conv (decoder block 4 conv2) on wgrad_c16.hip's fp16x3 kernel: from UWM_PREC_F16X3_ALL on
static bool c16_wg16_on(const uwm_model* m, size_t ci) {
  static const bool off = dbg_flag("UWM_NO_C16_WG16");
  const ConvL& cv = m->convs[ci];
  return !off && m->plan.prec >= UWM_PREC_F16X3_ALL && cv.bn >= 0 && cv.k == 3 && cv.stride == 1 && cv.CinP == 16 && cv.CoutP == 16 && cv.Cout == 16 && !cv.dw;
}
// ConvArgs::ig16 of conv ci's forward / dgrad launch: the fp16x3 forms that are not the direct 3x3 kernel
static bool conv_ig16(const uwm_model* m, size_t ci, bool dgrad) {
  return ig16_on(m, ci, dgrad) || up2_f16_on(m, ci, dgrad) || c16_f16_on(m, ci, dgrad);
}
// conv ci's weight gradient runs in fp16x3 (WgradArgs::prec = 2): the direct 3x3 kernel, or a dedicated kernel's fp16x3 form
static bool wgrad_f16_on(const uwm_model* m, size_t ci) {
  return f3_wgrad_on(m, ci) || ig16_on(m, ci, true) || up2_f16_on(m, ci, true) || stem_wg16_on(m, ci) || c16_wg16_on(m, ci);
}
// split products per tile (ConvArgs::nprod / WgradArgs::nprod) under the handle's precision mode: f16x1 = hi*hi' everywhere;
// f16x3_bwd2 = the backward's dY operand as ONE fp16 (two products), forward unchanged; the fp32-class modes: three
static int f3_nprod(const uwm_model* m, bool backward) {
  const int pm = m->plan.prec;
  if (pm == UWM_PREC_F16X1) return 1;
  if (pm == UWM_PREC_F16X3_BWD2 && backward) return 2;
  return 3;
}
// layout of a layer's fp16x3 bank (ConvArgs::wu_layout): 1 = conv_f16x3v2.hip (32x32x16 MFMA, 8 x 32-pixel tiles) where the map is
// tiled by whole tiles and the output rows by 32-row fragments (never a decoder conv1 dgrad: that kernel has no fused concat split)
static int f3_layout(const uwm_model* m, size_t ci, bool dgrad) {
  const ConvL& cv = m->convs[ci]; const Plan& p = m->plan;
  const int rows = dgrad ? cv.CinP : cv.Cout, chans = dgrad ? cv.CoutP : cv.CinP;
  if (rows != (dgrad ? cv.CinP : cv.CoutP)) return 0;
  if (dgrad && conv1_of(m, ci).block >= 0) return 0;
  return f16x3v2_shape(p.oh[ci], p.ow[ci], rows, chans) ? 1 : 0;
}
// everything the choice of a dgrad filter bank's FORM depends on (Winograd mode, precision mode, fp16x3 fill rule, routing batch):
// a change between a forward and its backward re-packs the banks at the start of the backward
static int pack_key(const uwm_model* m) {
  return ((m->plan.wino_mode * 8 + m->plan.prec) * 4099 + (m->f3_min_wgs & 0xfff)) * 257 + (m->route_n & 0xff);
}
// The FORM of the bank conv ci's forward slot holds under the current plan and modes; 0 = the slot is not used.  It mirrors what
// wino_jobs(dgrad = false) and the stem bank builder of do_forward make: 1 fp32 Winograd, 2 bf16x3 Winograd, 3 / 4 fp16x3 in conv_f16x3 /
// conv_f16x3v2 layout, 5 the stem's fp16x3 bank, 6 the implicit GEMM's pre-split weight operand.  uwm_freeze records it per layer; an eval forward reads the frozen arena only when
// every layer's form is the recorded one.
static int fwd_bank_form(const uwm_model* m, size_t ci) {
  const ConvL& cv = m->convs[ci];
  if (!cv.wu_off) return 0;
  if (cv.stem7()) return stem_f3_on(m) ? 5 : 0;
  if (cv.igb() && !cv.wino()) return ig_bank_on(m, ci, false) ? 6 : 0;
  if (!m->plan.wino_ok(ci)) return 0;
  if (f3_fwd_on(m, ci)) return 3 + f3_layout(m, ci, false);
  return m->plan.prec == UWM_PREC_BF16X3_ALL && cv.x3() ? 2 : 1;
}
// this eval forward may take its BatchNorm scale / shift and banks from the frozen arena
static bool frozen_serves(const uwm_model* m) {
  if (!m->frozen || m->fz_form.size() != m->convs.size()) return false;
  for (size_t ci = 0; ci < m->convs.size(); ++ci) if (fwd_bank_form(m, ci) != m->fz_form[ci]) return false;
  return true;
}
