// Kernel routing of libuwm: conv_route / wgrad_route decide, as pure host functions, which kernel a conv-class (forward conv / dgrad) or a
// weight-gradient launch runs on; launch_conv / launch_wgrad are argument sanity, the route, one switch.  What has to agree with the routing
// reads it here: conv_epilogue_carries_bnb and the bnb_* / out_up argument contract are lookups of the routed kernel's capabilities.
#include "uwm_kernels.h"
#include <stdio.h>
#include <stdlib.h>

namespace uwm {

static int g_winograd = -1;
bool winograd_enabled() {
  if (g_winograd < 0) { const char* e = getenv("UWM_WINOGRAD"); g_winograd = (e && e[0] == '0') ? 0 : 1; }
  return g_winograd != 0;
}
void winograd_set_mode(int mode) { g_winograd = mode; }
int winograd_mode() { (void)winograd_enabled(); return g_winograd; }
int device_cu_count() {
  static int cus[64] = {0};
  int dev = 0; (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) return 256;
  if (!cus[dev] && (hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus[dev] <= 0)) cus[dev] = 256;
  return cus[dev];
}

// the routing debug switches (all "unset" without UWM_DEBUG=1), read once
struct RouteSwitches {
  bool trace = dbg_flag("UWM_TRACE_CONV");
  bool no_up2 = dbg_flag("UWM_NO_UP2"), no_up2_wgrad = dbg_flag("UWM_NO_UP2_WGRAD"), no_head = dbg_flag("UWM_NO_CONV_HEAD");
  bool no_bnb_y = dbg_flag("UWM_NO_BNB_Y"), no_igemm_bnb = dbg_flag("UWM_NO_IGEMM_BNB");
  bool no_narrow_1x1 = dbg_flag("UWM_NO_NARROW_1X1"), no_wgrad_ig16 = dbg_flag("UWM_NO_WGRAD_IG16");
};
static const RouteSwitches& switches() { static const RouteSwitches s; return s; }

// What a kernel's epilogue can do with the fused BatchNorm-backward sums (ConvArgs::bnb_*) and the fused concat split (out_up): the
// sums | the sums with yhat from bnb_y | out_up | the sums beside out_up
struct ConvCaps { bool bnb, bnb_y, out_up, bnb_out_up; };
static ConvCaps conv_caps(ConvKernel k) {
  switch (k) {
    case kConvWino:         return {true, true, true, true};
    case kConvWinoX3:       return {true, false, true, true};
    // the fp16x3 epilogue could carry the sums beside the concat split; deliberately OFF: turning it on moves dgamma / dbeta of the
    // decoder BatchNorms from bn_bwd_reduce into the dgrad epilogue, i.e. changes the bits of a training step
    case kConvF16x3:        return {true, true, true, false};
    case kConvUp2Dgrad: case kConvUp2DgradF16: return {true, false, true, true};
    case kConvF16x3v2: case kConvGemm: case kConvS2Dgrad: case kConvIgemm: return {true, true, false, false};
    case kConvC16F16: case kConvC32F16: case kConvPatch16: case kConvHeadDgrad: return {true, false, false, false};
    default:                return {false, false, false, false};      // conv_up2 / conv_head (forward only), conv_wino8, conv_patch
  }
}
// force_cfg (uwm_op_conv's cfg, include/uwm.h): -1 = auto; every other accepted code is decoded here
ConvRoute conv_route(const ConvArgs& a, int cfg) {
  const RouteSwitches& sw = switches();
  const bool aut = cfg < 0;
  const ConvRoute invalid = {kConvInvalid, 0};
  // Winograd F(2x2,3x3): the 8-wave variant has neither the fused sums nor the concat split
  auto wino = [&](int bn) -> ConvRoute {
    if (bn == 8 || (bn <= 0 && !a.bnb_mean && !a.bnb_y && !a.out_up && conv_wino8_applicable(a))) return {kConvWino8, 0};
    return {kConvWino, bn};
  };
  auto up2 = [&]() -> ConvRoute { return {a.ig16 ? kConvUp2F16 : kConvUp2, 0}; };
  if (cfg == 700) return up2();
  if (cfg == 710 || (aut && a.ig16 && a.prec != 2 && conv_c16_f16_applicable(a))) return {kConvC16F16, 0};      // 16 -> 16 at full resolution, fp16x3
  if (cfg == 711 || (aut && a.ig16 && a.prec != 2 && conv_c32_f16_applicable(a))) return {kConvC32F16, 0};      // 32 -> 32, fp16x3
  if (cfg >= 800 && cfg < 1000) return {kConvGemm, cfg - 800};
  if (cfg == 500) return {kConvHead, 0};
  if ((cfg >= 600 && cfg <= 607) || (aut && a.prec == 2)) {      // fp16x3 direct form: the bank behind a.wu decides the kernel file
    const int v = aut ? 0 : cfg - 600;
    if (a.wu_layout == 1) return (v == 4 || v == 6 || !conv_f16x3v2_applicable(a)) ? invalid : ConvRoute{kConvF16x3v2, v == 5};      // 605: its 4-wave kernel
    return (v >= 4 || !conv_f16x3_applicable(a)) ? invalid : ConvRoute{kConvF16x3, v};
  }
  if (cfg == 400) return {kConvWinoX3, 0};
  if (cfg >= 300) return cfg < 400 ? wino(cfg - 300) : invalid;
  if (a.out_up) {                                                  // fused concat split: Winograd epilogues (and the sub-pixel dgrad of conv_up2.hip)
    if (aut && !sw.no_up2 && conv_up2_dgrad_applicable(a)) return {a.ig16 ? kConvUp2DgradF16 : kConvUp2Dgrad, 0};
    if (a.prec == 1) return conv_wino_x3_applicable(a) ? ConvRoute{kConvWinoX3, 0} : invalid;
    return conv_wino_applicable(a) ? wino(0) : invalid;
  }
  if (cfg == 200) return {kConvPatch16, 0};
  if (aut && !sw.no_up2 && conv_up2_applicable(a)) return up2();      // sub-pixel decomposition: Winograd's 2.25x without transforms
  if (aut && !sw.no_head && conv_head_applicable(a)) return {kConvHead, 0};
  if (aut && !sw.no_head && conv_head_dgrad_applicable(a)) return {kConvHeadDgrad, 0};      // few channels -> <= 4 classes: HBM streaming kernel
  // 16-channel inputs at full resolution are HBM-bound: the one-barrier direct kernel beats the Winograd pipeline there
  if (aut && wino_mode_of(a.wino) != 0 && conv_wino_applicable(a) && !conv_patch16_applicable(a))
    return a.prec == 1 ? ConvRoute{kConvWinoX3, 0} : wino(0);      // prec 1: the bank behind a.wu is a bf16x3 one
  if (cfg >= 100) return {kConvPatch, cfg - 100};
  if (aut && conv_patch16_applicable(a)) return {kConvPatch16, 0};
  if (aut && conv_patch_applicable(a)) {
    // patch-tiled 3x3: pick the channel tile so the launch has >= 512 workgroups when it can
    const long sp = (long)route_N(a) * ((a.Ho + 7) / 8) * ((a.Wo + 15) / 16);
    int bn = a.Cout >= 128 ? 128 : (a.Cout > 32 ? 64 : (a.Cout > 16 ? 32 : 16));
    if (bn == 128 && sp * ((a.Cout + 127) / 128) < 512) bn = 64;
    return {kConvPatch, bn};
  }
  if (aut && conv_s2_dgrad_applicable(a)) {
    // the four classes carry 1 / 2 / 2 / 4 of a 3x3's taps, so the launch is as long as its four-tap class: when that class alone
    // has fewer 128-wide tiles than CUs (layer3 / layer4 at batch 16: 128 / 64 workgroups, 169 / 233 us), 64 x 64 tiles
    const long t128 = (long)((route_N(a) * (a.Ho >> 1) * (a.Wo >> 1) + 127) / 128) * ((a.Cout + 127) / 128);
    if (a.Cout > 64 && t128 < device_cu_count()) return {kConvS2Dgrad, 4};
    return {kConvS2Dgrad, a.Cout <= 64 ? 1 : 0};
  }
  if (aut && conv_gemm_preferred(a)) return {kConvGemm, 0};      // 1x1 / stride 1, Cin % 32 == 0: persistent LDS-DMA GEMM
  if (aut) {                                                     // flattened implicit GEMM: tile configuration from the shape
    const long tiles128 = (long)((route_M(a) + 127) / 128);
    if (a.Cout <= 16) cfg = 3;
    else if (a.Cout <= 32) cfg = 2;
    else if (a.Cout <= 64) cfg = (tiles128 >= 512) ? 1 : 4;
    else {
      const long b0 = tiles128 * ((a.Cout + 127) / 128);
      // 1x1 layers with channel counts like 144 or 192 (MBConv expand / project dgrad): the 128-wide tile pads them to 256;
      // the 64-wide tile wastes far fewer MFMAs and LDS reads
      const int pad128 = ((a.Cout + 127) / 128) * 128, pad64 = ((a.Cout + 63) / 64) * 64;
      if (!sw.no_narrow_1x1 && a.ntaps == 1 && pad128 * 100 > pad64 * 115 && tiles128 * (pad64 / 64) >= 512) cfg = 1;
      else if (b0 >= 512) cfg = 0;
      else if (tiles128 * ((a.Cout + 63) / 64) >= 512) cfg = 1;
      else cfg = 4;
    }
  }
  return cfg <= 5 ? ConvRoute{kConvIgemm, cfg} : invalid;
}

// true when launch_conv(a, st) ends on a kernel whose epilogue carries the fused BatchNorm-backward sums for these arguments
// (asked before bnb_mean is set; a.bnb_y / a.out_up already are)
bool conv_epilogue_carries_bnb(const ConvArgs& a) {
  const ConvKernel k = conv_route(a, -1).k;
  const ConvCaps c = conv_caps(k);
  if (a.out_up) return c.bnb_out_up && !a.bnb_y;
  if (a.bnb_y) return c.bnb_y && a.prec != 1 && !switches().no_bnb_y;      // (prec 1 = a bf16x3 bank: conv_wino_x3's answer wherever the launch ends)
  if (switches().no_igemm_bnb && (k == kConvGemm || k == kConvS2Dgrad || k == kConvIgemm)) return false;
  return c.bnb;
}

hipError_t launch_conv(const ConvArgs& a, hipStream_t st, int force_cfg) {
  if (a.M <= 0 || a.Cout <= 0 || (a.Cout & 3) || (a.Kpad & 31) || (a.Ctot & 3) || (a.C0 & 3)) return hipErrorInvalidValue;
  if (switches().trace)
    fprintf(stderr, "conv %s N=%d Ctot=%d(C0=%d up=%d) Cout=%d Ho=%d Wo=%d Hl=%d Wl=%d taps=%d smul=%d sdiv=%d wino=%d gflop=%.2f\n",
            a.rmul < 0 ? "dgrad" : "fwd", a.N, a.Ctot, a.C0, a.s0.up, a.Cout, a.Ho, a.Wo, a.Hl, a.Wl, a.ntaps, a.smul, a.sdiv,
            (int)(force_cfg < 0 && wino_mode_of(a.wino) != 0 && conv_wino_applicable(a)), a.flops * 1e-9);
  const ConvRoute r = conv_route(a, force_cfg);
  // argument contract of the fused sums and of the concat split, against the routed kernel's capabilities: a caller that disagrees
  // with the router gets an error, not a wrong dgamma (the shape rules of out_up stay in the *_applicable of the kernels that take it)
  const ConvCaps c = conv_caps(r.k);
  if (a.bnb_mean && (!c.bnb || (a.bnb_y && !c.bnb_y) || (a.out_up && !c.bnb_out_up) || !a.ssum || !a.ssq || !a.bnb_rstd ||
                     !(a.out_up ? a.up_mask : (a.bnb_y ? a.bnb_y : a.mask)) || a.up_accum))
    return hipErrorInvalidValue;
  if (a.out_up && (!c.out_up || ((a.Ho | a.Wo) & 1) || (a.up_c0 & 3) || a.up_c0 > a.Cout || a.addend || a.mask || a.bias || a.bnb_y ||
                   (a.ssum && !a.bnb_mean) || (a.up_c0 < a.Cout && !a.out)))
    return hipErrorInvalidValue;
  switch (r.k) {
    case kConvUp2:         return launch_conv_up2(a, st);
    case kConvUp2F16:      return launch_conv_up2_f16(a, st);
    case kConvUp2Dgrad:    return launch_conv_up2_dgrad(a, st);
    case kConvUp2DgradF16: return launch_conv_up2_dgrad_f16(a, st);
    case kConvC16F16:      return launch_conv_c16_f16(a, st);
    case kConvC32F16:      return launch_conv_c32_f16(a, st);
    case kConvGemm:        return launch_conv_gemm(a, st, r.v);
    case kConvHead:        return launch_conv_head(a, st);
    case kConvHeadDgrad:   return launch_conv_head_dgrad(a, st);
    case kConvF16x3:       return launch_conv_f16x3(a, st, r.v);
    case kConvF16x3v2:     return launch_conv_f16x3v2(a, st, r.v != 0);
    case kConvWinoX3:      return launch_conv_wino_x3(a, st);
    case kConvWino:        return launch_conv_wino(a, st, r.v);
    case kConvWino8:       return launch_conv_wino8(a, st);
    case kConvPatch16:     return launch_conv_patch16(a, st);
    case kConvPatch:       return launch_conv_patch(a, st, r.v);
    case kConvS2Dgrad:     return launch_conv_s2_dgrad(a, st, r.v);
    case kConvIgemm:       return launch_conv_igemm(a, st, r.v);
    default:               return hipErrorInvalidValue;
  }
}

// force_igemm (uwm_op_wgrad, include/uwm.h), low byte: 0 auto | 1 flattened implicit GEMM only | 2 no dedicated kernel but
// wgrad_patch | 4 wgrad_gemm.hip | 6 the fp16x3 dedicated kernels | 7 the flattened implicit GEMM in its fp16x3 form
WgradRoute wgrad_route(const WgradArgs& a) {
  const RouteSwitches& sw = switches();
  const int f = a.force_igemm & 0xff;
  const bool aut = f == 0, no_up2 = sw.no_up2 || sw.no_up2_wgrad;
  if (f == 4) return {kWgradGemm, 0};
  if (a.prec == 2 && (aut || f == 6)) {
    if (a.xmax && !no_up2 && wgrad_up2_applicable(a) && wgrad_up2_f16_shape(a)) return {kWgradUp2, 0};      // sub-pixel form of conv-after-upsample on its fp16x3 kernel (2.25x fewer products than the direct form below)
    if (wgrad_f16x3_applicable(a)) return {kWgradF16x3, 0};      // fp16x3 direct form
  }
  if (f == 6) {                                                  // (the fp16x3 kernels of wgrad_stem.hip / wgrad_c16.hip)
    if (a.prec == 2 && wgrad_stem_applicable(a)) return {kWgradStem, 0};
    if (a.prec == 2 && a.Cout == 16 && wgrad_c16_applicable(a)) return {kWgradC16, 0};
    return {kWgradInvalid, 0};
  }
  if (aut && !no_up2 && wgrad_up2_applicable(a)) return {kWgradUp2, 0};      // sub-pixel form of conv-after-upsample
  if (aut && wgrad_stem_applicable(a)) return {kWgradStem, 0};               // the ResNet stem: compact K = 147
  if (aut && wgrad_gemm_preferred(a)) return {kWgradGemm, 0};                // 1x1 / stride 1: persistent LDS-DMA GEMM, deterministic
  if (aut && wgrad_c16_applicable(a)) return {kWgradC16, 0};                 // 16-channel full-resolution layers, head
  if (aut && wino_mode_of(a.wino) != 0 && wgrad_wino_applicable(a)) return {kWgradWino, 0};
  if (f != 1 && f != 7 && wgrad_patch_applicable(a)) return {kWgradPatch, 0};
  // flattened implicit GEMM; v = 1: its fp16x3 form where the tile has one (the stride-2 layers in the f16x3_all modes; channel counts in whole 32s)
  const bool f16 = !sw.no_wgrad_ig16 && a.prec == 2 && a.xmax && (aut || f == 7) && (a.Ctot & 31) == 0 && (a.Cout & 31) == 0;
  return {kWgradIgemm, f16 ? 1 : 0};
}

hipError_t launch_wgrad(const WgradArgs& a, hipStream_t st) {
  if (switches().trace)
    fprintf(stderr, "wgrad N=%d Ctot=%d(C0=%d) Cout=%d wrows=%d Ho=%d Wo=%d Hl=%d Wl=%d taps=%d stride=%d wino=%d patch=%d gflop=%.2f\n", a.N, a.Ctot,
            a.C0, a.Cout, a.wrows, a.Ho, a.Wo, a.Hl, a.Wl, a.ntaps, a.stride, (int)(wino_mode_of(a.wino) != 0 && wgrad_wino_applicable(a)),
            (int)wgrad_patch_applicable(a), a.flops * 1e-9);
  const WgradRoute r = wgrad_route(a);
  switch (r.k) {
    case kWgradGemm:  return launch_wgrad_gemm(a, st);
    case kWgradUp2:   return launch_wgrad_up2(a, st);
    case kWgradF16x3: return launch_wgrad_f16x3(a, st);
    case kWgradStem:  return launch_wgrad_stem(a, st);
    case kWgradC16:   return launch_wgrad_c16(a, st);
    case kWgradWino:  return launch_wgrad_wino(a, st);
    case kWgradPatch: return launch_wgrad_patch(a, st);
    case kWgradIgemm: return launch_wgrad_igemm(a, st, r.v != 0);
    default:          return hipErrorInvalidValue;
  }
}

}  // namespace uwm
