// Internal kernel-launch interface of libuwm (MI355X / gfx950 only).
// Layout conventions:
//   activations  NHWC fp32, channel count padded to a multiple of 4
//   weights      [Cout_rows][Kpad] fp32, k = tap*Ctot + c  (tap = r*kw + s), Kpad % 32 == 0
//   a "lazy" activation = raw conv output + per-channel (scale, shift[, relu]) applied by
//   the CONSUMER when it stages the tile (BatchNorm-apply + ReLU never make their own pass)
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>

struct uwm_loss_spec;        // include/uwm.h

namespace uwm {

struct Src {                 // one (possibly lazily transformed) NHWC activation
  const float* ptr;          // [N][H][W][C]
  const float* scale;        // per-channel scale or nullptr (identity)
  const float* shift;        // per-channel shift (valid when scale != nullptr)
  int C, H, W;               // physical dims
  int up;                    // log2 nearest-upsample factor seen by the consumer (0|1)
  int relu;                  // max(.,0) after the affine
};

struct FastDiv {             // n / d for n*d < 2^32 (k-index arithmetic only)
  unsigned mg, d;
};
static inline FastDiv make_fastdiv(unsigned d) {
  FastDiv f; f.d = d; f.mg = (d <= 1) ? 0u : (unsigned)((0x100000000ull / d) + 1ull); return f;
}

// ---- per-device launch state.  hipFuncSetAttribute and the CU count belong to a DEVICE, not to the process: one flag
// per (kernel instantiation, device), so a process that drives several GPUs sets the attribute on each of them.
struct DevOnce {
  std::atomic<unsigned long long> mask{0};          // one host thread per GPU may race here: the attribute call is idempotent, the bit set is atomic
  hipError_t set_max_lds(const void* fn, size_t bytes) {
    int dev = 0; hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 64 && ((mask.load(std::memory_order_acquire) >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && dev < 64) mask.fetch_or(1ull << dev, std::memory_order_release);
    return e;
  }
};
// ---- debug switches: ONE gate.  Every routing / ablation switch of the library (UWM_NO_*, UWM_TRACE_CONV, UWM_WW_TA:
// INTEGRATION.md 2b) is read through dbg_flag() / dbg_int(), which answer "unset" unless UWM_DEBUG=1 is in the environment — a
// production process cannot be re-routed by a stray variable.  (UWM_WINOGRAD and UWM_SIDE_STREAM are documented process
// defaults of public setters, not debug switches.)
bool dbg_flag(const char* name);                // UWM_DEBUG=1 and `name` set
int dbg_int(const char* name, int dflt);        // UWM_DEBUG=1 and `name` set ? atoi : dflt
int device_cu_count();       // compute units of the CURRENT device (cached per device)

struct ConvArgs {            // implicit-GEMM conv: forward conv AND dgrad (transposed gather)
  Src s0, s1;                // channel-concat of two sources: [0,C0) from s0, [C0,Ctot) from s1
  int C0, Ctot;
  const float* w;            // [wrows][Kpad]
  int wrows, Kpad, ntaps, kw;
  int N, Ho, Wo, Cout, M;    // output [N][Ho][Wo][Cout], M = N*Ho*Wo
  int Hl, Wl;                // logical (post-upsample) input dims used for the bounds check
  int smul, rmul, off, sdiv; // hi_num = ho*smul + r*rmul + off ; hi = hi_num / sdiv (must divide)
  float* out;
  const float* bias;         // [Cout] or nullptr
  const float* addend;       // [M][Cout] added in the epilogue or nullptr
  const float* mask;         // [M][Cout]: out = (mask*mscale+mshift > 0) ? out : 0, or nullptr
  const float* mscale; const float* mshift;
  double* ssum; double* ssq; // per-channel sum / sum of squares of the output, or nullptr
  int srep, sstride;         // statistics replicas: workgroup b adds into copy (b & (srep-1)) at +copy*sstride doubles (srep: power of 2, 0/1 = none)
  // BatchNorm-backward sums fused into a dgrad epilogue (conv_wino.hip / conv_wino_x3.hip only; bnb_mean != nullptr): the
  // epilogue's masked output v IS the gradient wrt a BatchNorm output whose raw input it has just read as the ReLU mask
  // (`mask` / `up_mask`), so it accumulates ssum += v (dbeta) and ssq += v * (mask_raw - mean) * rstd (dgamma) instead of the
  // forward's (v, v^2): bn_bwd_reduce's pass over both tensors disappears
  const float* bnb_mean; const float* bnb_rstd;
  // bnb_y != nullptr: yhat is taken from THIS tensor (same [M][Cout] indexing as the output) instead of the mask tensor: the dgrad
  // that writes the gradient wrt a residual block's OUTPUT (masked by that output) carries the sums of the block's last BatchNorm,
  // whose raw input is a different tensor (conv_wino_kernel<NI> plain epilogue and conv_igemm_kernel only)
  const float* bnb_y;
  FastDiv dv_ctot, dv_kw;
  double flops;              // algorithmic FLOPs of this launch (host-side profiling only)
  double bytes;              // algorithmic HBM bytes of this launch: every operand read once + the output written once (profiling only)
  // decoder dgrad with the concat split fused into the epilogue (conv_wino.hip only): output channels [0, up_c0) are
  // summed over each 2x2 pixel block (nearest-x2 upsample backward), ReLU-masked by the low-resolution producer
  // (up_mask * up_mscale + up_mshift > 0) and written to out_up [N][Ho/2][Wo/2][up_c0]; channels [up_c0, Cout) go to
  // `out` as [N][Ho][Wo][Cout - up_c0] (may be nullptr when there are none)
  float* out_up; int up_c0; const float* up_mask; const float* up_mscale; const float* up_mshift;
  int up_accum;              // out_up += instead of = (a tensor with several consumers: UNet++)
  int pc_ntaps[4]; unsigned pc_taps[4];          // stride-2 dgrad parity classes (conv_igemm.hip; blockIdx.y = class), set by the launcher
  int live_ch;               // dgrad: channels of dY that can be non-zero (0 = all; the head's classes inside its 4 padded channels)
  const float* wu;           // Winograd-transformed weights (conv_wino.hip layout) or nullptr
  int wu_ncb;                // 16-row blocks per xi in wu
  int wino;                  // Winograd mode of this launch: 0 = process default (uwm_set_winograd), else mode + 1 (per-handle: uwm_set_winograd_mode)
  int prec;                  // 1: wu is a bf16x3 bank (conv_wino_x3.hip layout) and the launch goes to the split-bf16 kernel; 2: wu is an fp16x3 bank (conv_f16x3.hip: direct form on v_mfma_f32_16x16x32_f16, fp32-class accuracy); 0: fp32
  int wu_rinv_off;           // prec 2: float offset of the bank's 1 / row-scale array from wu
  const float* xmax;         // prec 2: 32 device floats whose maximum is max|input| (a dgrad's dY, written by bn_bwd_apply), or nullptr: the input is staged times the power of two that puts that maximum in [2^13, 2^14), undone in the epilogue
  int route_n;               // > 0: choose the kernel VARIANT as if the batch were route_n images (uwm_set_routing_batch: a small parity sample on the kernels the full batch takes); 0: N
  int ig16;                  // implicit-GEMM launches (conv_igemm.hip: stride-2 3x3, 1x1 stride 2, their dgrads) and the sub-pixel decoder conv (conv_up2_f16.hip): 1 = fp16x3 split products on v_mfma_f32_16x16x32_f16 (operands split while staging, weights times 2^12, a dgrad's dY by xmax); 0 = exact fp32
  int nprod;                 // prec 2: split products per tile — 0 / 3: hi*hi' + hi*lo' + lo*hi' (fp32-class); 2: the pixel operand (a dgrad's dY) as ONE fp16 (hi*hi' + lo_w*hi'); 1: hi*hi' only (plain fp16 products, the reference's autocast arithmetic)
  // ig16 launches of conv_igemm.hip: w pre-split once per step (ig_bank_unit below, built inside the multi-job bank
  // launches) — same [wrows][Kpad] indexing, every 32-float chunk replaced by its 128-byte LDS row image; nullptr = split while staging
  const float* wbank;
  int wu_layout;             // prec 2: layout of the fp16x3 bank behind wu — 0: conv_f16x3.hip (tap pairs, 16-row fragments), 1: conv_f16x3v2.hip (taps, 32-row fragments); set by whoever packed the bank (f16x3v2_shape)
};

// batch the VARIANT choice of a launcher is made for (ConvArgs::route_n / WgradArgs::route_n; grids always use the real N)
template <class A> static inline int route_N(const A& a) { return a.route_n > 0 ? a.route_n : a.N; }
template <class A> static inline long route_M(const A& a) { return a.N > 0 ? (long)a.M / a.N * route_N(a) : (long)a.M; }

#if defined(__HIPCC__)
// ---- device helpers the convolution and weight-gradient kernels share ----
typedef _Float16 uwm_h8 __attribute__((ext_vector_type(8)));

// Power-of-two range scale of the fp16x3 arithmetic: the factor 2^(14 - e) that puts a maximum mx = m * 2^e (m in [0.5, 1)) into
// [2^13, 2^14) — high in fp16's range (largest finite value 65504), so the hi / lo halves of the small values beside it stay
// normal numbers.  Exact (a power of two), undone in the epilogue.  1 for a zero, infinite or NaN maximum.
__device__ __forceinline__ float uwm_pow2_scale(float mx) {
  float s = 1.f;
  if (mx > 0.f && mx < 3.0e38f) { int e; (void)frexpf(mx, &e); s = ldexpf(1.f, 14 - e); }
  return s;
}
// Range scale of a dgrad's dY: max|dY| = the maximum of the 32 floats at xmax (ConvArgs::xmax, filled by bn_bwd_apply), every
// lane of the wave gets the same value (32-lane butterfly; workgroups are one-dimensional).  xmax is not null: whether a launch
// scales at all is the caller's guard.  The lane index is taken here, not passed in: handing the kernel's `lane` through a
// parameter changed the instruction order of wgrad_f16x3_kernel<16> and wgrad_stem_f16_kernel (scripts/isa_identity.py).
__device__ __forceinline__ float uwm_dy_scale(const float* xmax) {
  float mx = xmax[threadIdx.x & 31];
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  return uwm_pow2_scale(mx);
}
// XCD-aware walk: the hardware deals workgroups round-robin over the 8 XCDs, so consecutive blockIdx.x values — neighbouring tiles
// that stream the SAME operand block — land on eight different L2s and fetch it eight times (wgrad_f16x3, PMC: 235 MB fetched
// per launch against 83 MB algorithmic).  This bijective remap of blockIdx.x gives every XCD a contiguous range of the linear
// tile order (the first gridDim.x % 8 XCDs one tile more), so the tiles that share an operand meet in one L2.
__device__ __forceinline__ unsigned uwm_xcd_tile() {
  const unsigned nblk = gridDim.x, bid = blockIdx.x;
  const unsigned q8 = nblk >> 3, r8 = nblk & 7, xcd = bid & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}
// Two transposed LDS reads (ds_read_b64_tr_b16: a 4 x 16 block of halfs per 16 lanes, delivered column-major) joined into one
// 8-half MFMA operand fragment
__device__ __forceinline__ uwm_h8 uwm_tr_pair(const char* base, int o0, int o1) {
  typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
  typedef __fp16 fp16x8 __attribute__((__vector_size__(8 * sizeof(__fp16))));
  typedef __attribute__((address_space(3))) fp16x4 lds_fp16x4;
  const fp16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4*)(uintptr_t)(base + o0));
  const fp16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4*)(uintptr_t)(base + o1));
  const fp16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(uwm_h8, v);
}
// Clamp to fp16's finite range in one v_med3_f32 (fminf(fmaxf()) adds a canonicalising v_max per value)
__device__ __forceinline__ float uwm_clamp_h(float v) { return __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f); }

// Split of four fp32 values into hi / lo fp16 halves (the fp16x3 operand form): hi = rn_f16(x) (v_cvt_pk_f16_f32, two values per
// instruction), lo = rn_f16(x - hi) as ONE v_fma_mix{lo,hi}_f16 per value — fma(hi_as_f32, -1.0, x) rounded to fp16 into one half
// of the destination, the fp16 operand selected out of the packed register by op_sel (exact: an fp32 value minus its fp16 rounding
// is representable in fp32).  Results as packed pairs: {x, y}, {z, w}.
typedef unsigned uwm_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void uwm_split4(float x0, float x1, float x2, float x3, uwm_u2& hi, uwm_u2& lo) {
  typedef _Float16 h2_ __attribute__((ext_vector_type(2)));
  const h2_ a = {(_Float16)x0, (_Float16)x1}, b = {(_Float16)x2, (_Float16)x3};
  hi.x = __builtin_bit_cast(unsigned, a); hi.y = __builtin_bit_cast(unsigned, b);
  unsigned l0, l1;
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(l0) : "v"(hi.x), "v"(x0), "v"(x1));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(l1) : "v"(hi.y), "v"(x2), "v"(x3));
  lo.x = l0; lo.y = l1;
}
// ... of values that may leave fp16's range (weights times their scale, raw activations): clamped first, so hi stays finite
__device__ __forceinline__ void uwm_split4_clamped(float x0, float x1, float x2, float x3, uwm_u2& hi, uwm_u2& lo) {
  uwm_split4(uwm_clamp_h(x0), uwm_clamp_h(x1), uwm_clamp_h(x2), uwm_clamp_h(x3), hi, lo);
}
// The weight operand of conv_igemm.hip's fp16x3 form, pre-split: unit i = floats [4i, 4i + 4) of a [rows][Kpad] matrix (Kpad % 32 == 0)
// goes times 2^12, clamped, as hi / lo fp16 halves to its place in the 128-byte LDS row image of its 32-float chunk (32 hi halfs |
// 32 lo halfs, 16-byte slots XOR-swizzled by (row >> 1) & 7) — the very arithmetic and layout of conv_igemm_kernel's staging code,
// so a banked launch copies 16 bytes per thread and every product is bit-identical to the on-the-fly split's.
constexpr float kIgWScale = 4096.f;
__device__ __forceinline__ void ig_bank_unit(const float* __restrict__ src, float* __restrict__ dst, size_t i, int Kpad) {
  typedef float f4_ __attribute__((ext_vector_type(4)));
  const size_t g = i >> 3;                             // 32-float chunk
  const int unit = (int)(i & 7), row = (int)((g * 32) / (size_t)Kpad);
  const f4_ w4 = *(const f4_*)(src + i * 4) * kIgWScale;
  uwm_u2 hi, lo;
  uwm_split4_clamped(w4.x, w4.y, w4.z, w4.w, hi, lo);
  char* rb = (char*)(dst + g * 32);
  const int sw = (row >> 1) & 7;
  *(uwm_u2*)(rb + (((unit >> 1) ^ sw) << 4) + (unit & 1) * 8) = hi;
  *(uwm_u2*)(rb + ((((unit >> 1) + 4) ^ sw) << 4) + (unit & 1) * 8) = lo;
}
#endif

// Deferred partial-sum reduces.  A split weight-gradient launch leaves `nsplit` dW-shaped partial images in scratch; adding them
// up (fixed order) used to be one small launch behind every wgrad (37 per resnet34 step, each 3x slower beside the other
// stream's kernels than alone).  With a queue attached (WgradArgs::rq) the launcher only records the job; the owner flushes the
// queue with ONE multi-job launch per backward stage (launch_wgrad_reduce_multi) — same arithmetic per job, so the result is
// bit-identical to the immediate form.  The owner hands every queued job its own scratch region (rq->used_floats).
struct ReduceJob { const float* part; float* dw; unsigned long long n4; int nsplit; unsigned block0; };
struct ReduceQueue {
  enum { kMax = 48 };
  ReduceJob j[kMax]; int n = 0; unsigned blocks = 0; size_t used_floats = 0;
};
struct ReduceJobs { ReduceJob j[ReduceQueue::kMax]; int n; };

struct WgradArgs {           // dW[co][k] += sum_m dY[m][co] * X[m][k]   (k = tap*Ctot + c)
  Src s0, s1; int C0, Ctot;
  const float* dy;           // [M][Cout]
  float* dw;                 // [wrows][Kpad], accumulated with float atomics
  int wrows, Kpad, ntaps, kw;
  int N, Ho, Wo, Cout, M;
  int Hl, Wl, stride, pad;
  int nsplit, msplit;        // pixel range per split (multiple of 32)
  float* part;               // scratch for per-split partial dW tiles (Winograd wgrad: deterministic two-stage sum) or nullptr
  size_t part_floats;        // its capacity
  int force_igemm;           // tests: 1 = never route to wgrad_patch
  FastDiv dv_ctot, dv_kw;
  double flops;              // algorithmic FLOPs of this launch (host-side profiling only)
  double bytes;              // algorithmic HBM bytes of this launch: every operand read once + the output written once (profiling only)
  int wino;                  // as ConvArgs::wino
  int prec;                  // 2: fp16x3 direct weight gradient (wgrad_f16x3.hip) where applicable; 0: fp32 kernels
  const float* xmax;         // prec 2: 32 device floats whose maximum is max|dy| (written by bn_bwd_apply): dY is staged times the power of two that puts it in [2^13, 2^14)
  ReduceQueue* rq;           // HOST pointer (never read on the device) or nullptr: queue the partial-sum reduce instead of launching it
  int cu_share;              // prec 2: 0 = one workgroup per CU; n = per n/4 of the CUs (3 when the launch runs beside the dependent chain: the rest stay free of its 768-thread workgroups)
  int route_n;               // as ConvArgs::route_n
  int nprod;                 // prec 2: as ConvArgs::nprod (2: dY as one fp16: dy_hi*x_hi + dy_hi*x_lo)
};

// ---- optional HIP-event profiler: one (start, stop) event pair per conv / wgrad launch, recorded on
// the launch stream; classes 0..5 = conv_igemm tile configs, 6..9 = wgrad tiles 64x128, 128x128, 16x256, 32x256,
// 10..13 = conv_patch BN 128, 64, 32, 16 ; 14..16 = wgrad_patch TA 16, 32, 64 ; 17..18 = conv_patch16 BN 16, 32
enum { kProfClasses = 64 };   // 60..62 = wgrad_igemm_f16x3 tiles 128x128, 128x64, 64x128 ; 45 = conv_up2_f16x3 ; 46 = conv_up2_dgrad_f16x3 ; 47 = wgrad_up2_f16x3 ; 48 = conv_c16_f16x3 ; 49 = wgrad_c16_f16x3 ; 50 = wgrad_stem_f16x3 ; 51..52 = conv_gemm_f16x3 BN 128, 64 ; 53..58 = conv_igemm_f16x3 tile configurations 0..5 ; 44 = conv_stem_f16x3 ; 43 = wgrad_f16x3 ; 42 = conv_f16x3 ; 41 = wgrad_stem ; 39..40 = wgrad_gemm TA 128, 64 ; 37..38 = conv_gemm BN 128, 64 ; 34 = conv_up2 ; 35 = conv_up2_dgrad ; 36 = wgrad_up2 ; 31 = conv_wino_x3 (bf16x3) ; 32 = wgrad_c16 ; 33 = wgrad_head ; 19..21 = conv_wino BN 64, 32, 16 ; 22..24 = wgrad_wino TA 64, 32, 16 ; 25 = conv_wino8 ; 26..29 = wgrad tiles 128x32, 128x64, 32x64, 32x128 ; 30 = conv_head
void prof_enable(bool on);
bool prof_on();
void prof_pair(int cls, double flops, double bytes, hipEvent_t* e0, hipEvent_t* e1);
// routing record: every UWM_LAUNCH leaves the name of the kernel it dispatched in a thread-local slot; the model copies it into its
// per-handle routing log (uwm_routing_dump) so a test / bench.py can assert WHICH kernel a layer ran on
void route_note(const char* kernel);
const char* route_last();
// One profiled launch = one (start, stop) event pair attached to the KERNEL DISPATCH itself (hipExtLaunchKernelGGL): the
// pair carries the dispatch's own begin / end timestamps — the clock rocprofv3's kernel trace reads — so a launch that
// waits for CUs behind the other stream's kernels is not charged for the wait (events recorded AROUND the launch were).
#define UWM_LAUNCH(cls, flops, bytes, kernel, grid, block, lds, st, ...)                                     \
  do {                                                                                                       \
    route_note(#kernel);                                                                                     \
    if (prof_on()) {                                                                                         \
      hipEvent_t e0_, e1_; prof_pair((cls), (flops), (bytes), &e0_, &e1_);                                   \
      hipExtLaunchKernelGGL(kernel, grid, block, lds, st, e0_, e1_, 0, __VA_ARGS__);                         \
    } else {                                                                                                 \
      hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);                                         \
    }                                                                                                        \
  } while (0)
int  prof_collect(double* out /* [kProfClasses][4] = launches, ms, flops, bytes */);
const char* prof_class_name(int cls);

// ---- launchers (all asynchronous on `st`, no host sync, no allocation) ----
// Routing (uwm_route.hip): ONE decision per launch.  conv_route / wgrad_route are pure host functions (nothing of HIP but
// device_cu_count()); launch_conv / launch_wgrad are argument sanity, the route, one switch.  v = the variant / tile code the routed
// kernel's launcher takes (0 where it takes none).
enum ConvKernel { kConvInvalid = 0, kConvUp2, kConvUp2F16, kConvUp2Dgrad, kConvUp2DgradF16, kConvC16F16, kConvC32F16, kConvGemm, kConvHead,
                  kConvHeadDgrad, kConvF16x3, kConvF16x3v2, kConvWinoX3, kConvWino, kConvWino8, kConvPatch16, kConvPatch, kConvS2Dgrad, kConvIgemm };
struct ConvRoute { ConvKernel k; int v; };
ConvRoute conv_route(const ConvArgs& a, int force_cfg);      // force_cfg: uwm_op_conv's cfg (include/uwm.h lists every code); -1 = auto
hipError_t launch_conv(const ConvArgs& a, hipStream_t st, int force_cfg = -1);
bool conv_epilogue_carries_bnb(const ConvArgs& a);      // conv_route(a, -1) ends on a kernel whose epilogue carries the fused BatchNorm-backward sums (bnb_*) for these arguments; launch_conv REJECTS a.bnb_mean on every other kernel, so a disagreement with the router is an error, not a wrong dgamma
enum WgradKernel { kWgradInvalid = 0, kWgradGemm, kWgradUp2, kWgradF16x3, kWgradStem, kWgradC16, kWgradWino, kWgradPatch, kWgradIgemm };
struct WgradRoute { WgradKernel k; int v; };                 // v (kWgradIgemm): 1 = the fp16x3 form where the tile has one
WgradRoute wgrad_route(const WgradArgs& a);                  // WgradArgs::force_igemm: uwm_op_wgrad's (include/uwm.h)
hipError_t launch_wgrad(const WgradArgs& a, hipStream_t st);
// flattened implicit GEMM (conv_igemm.hip / wgrad_igemm.hip); tile configurations {BM, BN}: 0:{128,128} 1:{128,64} 2:{128,32} 3:{128,16} 4:{64,64} 5:{64,128}
hipError_t launch_conv_igemm(const ConvArgs& a, hipStream_t st, int cfg);
bool conv_s2_dgrad_applicable(const ConvArgs& a);            // stride-2 dgrad as four parity-class launches
hipError_t launch_conv_s2_dgrad(const ConvArgs& a, hipStream_t st, int cfg);      // cfg 0 | 1 | 4
hipError_t launch_wgrad_igemm(const WgradArgs& a, hipStream_t st, bool f16);       // tile and split from the shape
// 3x3 s1 p1 patch-tiled conv (conv_patch.hip); launch_conv routes to it when applicable.
bool wgrad_patch_applicable(const WgradArgs& a);
hipError_t launch_wgrad_patch(const WgradArgs& a, hipStream_t st);
bool wgrad_wino_applicable(const WgradArgs& a);            // Winograd-domain wgrad (wgrad_wino.hip)
hipError_t launch_wgrad_wino(const WgradArgs& a, hipStream_t st);
size_t wgrad_wino_scratch_floats();                         // workspace the model plans for WgradArgs::part
float* wgrad_op_scratch();                                  // the same, for the single-operator entry points (cached per device)
bool wgrad_c16_applicable(const WgradArgs& a);              // 16-channel full-resolution layers and the head (wgrad_c16.hip)
hipError_t launch_wgrad_c16(const WgradArgs& a, hipStream_t st);
hipError_t launch_wgrad_reduce(const float* part, int nsplit, size_t n4, float* dw, hipStream_t st, ReduceQueue* rq = nullptr);      // dw += sum of nsplit full-size partial images, fixed order; rq: queued, not launched
hipError_t launch_wgrad_reduce_multi(ReduceQueue& q, hipStream_t st);        // every queued job in one launch; empties the queue
bool wgrad_f16x3_applicable(const WgradArgs& a);            // fp16x3 direct weight gradient of the 3x3 / stride-1 layers (wgrad_f16x3.hip); needs a.xmax
hipError_t launch_wgrad_f16x3(const WgradArgs& a, hipStream_t st);
bool wgrad_stem_applicable(const WgradArgs& a);             // 7x7 / stride-2 / 3(4)-channel stem: compact-column wgrad (wgrad_stem.hip)
hipError_t launch_wgrad_stem(const WgradArgs& a, hipStream_t st);
bool wgrad_gemm_applicable(const WgradArgs& a);             // 1x1 / stride-1 weight gradient as a persistent LDS-DMA GEMM (wgrad_gemm.hip)
hipError_t launch_wgrad_gemm(const WgradArgs& a, hipStream_t st);
bool wgrad_gemm_preferred(const WgradArgs& a);            // applicable AND not a many-pixel / tiny-dW layer (those stay on wgrad_igemm)
bool wgrad_up2_applicable(const WgradArgs& a);              // wgrad of conv_up2.hip's layer (nearest-x2 upsampled 32-channel input, 16 outputs)
hipError_t launch_wgrad_up2(const WgradArgs& a, hipStream_t st);
bool conv_gemm_applicable(const ConvArgs& a);             // 1x1 / stride-1 conv as a persistent LDS-DMA GEMM (conv_gemm.hip); force_cfg 800 (auto tile) / 864 / 928
hipError_t launch_conv_gemm(const ConvArgs& a, hipStream_t st, int bn);
bool conv_gemm_preferred(const ConvArgs& a);              // applicable AND enough tiles to fill the chip (else the implicit GEMM's 64x64 tiles)
bool conv_up2_applicable(const ConvArgs& a);              // 3x3 over a nearest-x2 upsampled 32-channel input, 16 outputs (conv_up2.hip)
hipError_t launch_conv_up2(const ConvArgs& a, hipStream_t st);
bool conv_up2_dgrad_applicable(const ConvArgs& a);        // its dgrad wrt the low-resolution input, concat-split epilogue contract (ConvArgs::out_up)
hipError_t launch_conv_up2_dgrad(const ConvArgs& a, hipStream_t st);
// conv_up2_f16.hip: the same two launches on v_mfma_f32_16x16x32_f16 with fp16x3 split products (conv_route takes them when ConvArgs::ig16 is set)
hipError_t launch_conv_up2_f16(const ConvArgs& a, hipStream_t st);
hipError_t launch_conv_up2_dgrad_f16(const ConvArgs& a, hipStream_t st);
// conv_c16_f16.hip: 3x3 from 16 to 16 channels at full resolution (decoder block 4 conv2), forward and dgrad, fp16x3 (taken when ConvArgs::ig16 is set); force_cfg 710
bool conv_c16_f16_applicable(const ConvArgs& a);
hipError_t launch_conv_c16_f16(const ConvArgs& a, hipStream_t st);
bool conv_c32_f16_applicable(const ConvArgs& a);          // the same for 32 -> 32 channels (decoder block 3 conv2); force_cfg 711
hipError_t launch_conv_c32_f16(const ConvArgs& a, hipStream_t st);
bool wgrad_up2_f16_shape(const WgradArgs& a);             // its weight gradient: 2 x 32 low-resolution tiles
int wgrad_up2_f16_parts(const WgradArgs& a);              // workgroup partials of that launch (wgrad_up2_kernel's layout)
hipError_t launch_wgrad_up2_f16(const WgradArgs& a, hipStream_t st);
bool conv_patch_applicable(const ConvArgs& a);
bool conv_patch16_applicable(const ConvArgs& a);          // 16-channel inputs: whole K in LDS (conv_patch16.hip)
hipError_t launch_conv_patch16(const ConvArgs& a, hipStream_t st);
hipError_t launch_conv_patch(const ConvArgs& a, hipStream_t st, int bn);
// Winograd F(2x2,3x3) (conv_wino.hip): needs a.wu = launch_wino_weights(a.w ...) output; force_cfg 300 (auto tile) / 300+BN
bool conv_wino_applicable(const ConvArgs& a);
hipError_t launch_conv_wino(const ConvArgs& a, hipStream_t st, int bn = 0);   // bn: 0 auto | 64 | 32 | 16 (the 8-wave variant: launch_conv_wino8)
// segmentation head (3x3, 8|16|32 channels -> <= 4 classes, bias): HBM streaming kernel (conv_head.hip); force_cfg 500
bool conv_head_applicable(const ConvArgs& a);
hipError_t launch_conv_head(const ConvArgs& a, hipStream_t st);
bool conv_head_dgrad_applicable(const ConvArgs& a);          // its dgrad (4 padded classes -> 8|16|32 channels, ReLU mask)
hipError_t launch_conv_head_dgrad(const ConvArgs& a, hipStream_t st);
bool conv_wino8_applicable(const ConvArgs& a);              // 512-thread, 16x16-pixel, 64-channel variant (conv_wino8.hip)
hipError_t launch_conv_wino8(const ConvArgs& a, hipStream_t st);
size_t wino_weights_floats(int wrows, int Ctot);
int wino_ncb(int wrows);
hipError_t launch_wino_weights(const float* w, int wrows, int Kpad, int Ctot, int mirror, float* ut, hipStream_t st);
struct WinoJob { const float* w; float* ut; int rows, chans, Kpad, mode, src_rows, pad_; };      // mode 3 (launch_f16x3_weights_multi only): ut = ig_bank_unit image of the [rows][Kpad] matrix w
struct WinoJobs { static constexpr int kMax = 56; WinoJob j[kMax]; int n; };      // (resnet34: 38 fp16x3 forward banks + 6 implicit-GEMM ones in ONE launch)
hipError_t launch_wino_weights_multi(const WinoJobs& jobs, hipStream_t st);   // every layer's transform in one launch
// bf16x3 precision mode (conv_wino_x3.hip): split-bf16 filter banks (same size as the fp32 ones) and the conv kernel; force_cfg 400
hipError_t launch_wino_weights_x3_multi(const WinoJobs& jobs, hipStream_t st);
// fp16x3 direct convolution (conv_f16x3.hip): split-fp16 filter banks and the conv kernel; force_cfg 600
int f16x3_nj(int rows);
size_t f16x3_bank_floats(int rows, int chans);             // bank size in floats, 1 / row-scale array included
size_t f16x3_rinv_off(int rows, int chans);                 // float offset of that array in the bank
hipError_t launch_f16x3_weights_multi(const WinoJobs& jobs, hipStream_t st);      // WinoJob::pad_ = bank layout (ConvArgs::wu_layout)
bool conv_f16x3_applicable(const ConvArgs& a);
static inline __host__ __device__ size_t f16x3_rinv_off_floats(int rows, int chans) { return (size_t)(chans / 16) * 5 * (size_t)(((rows + 63) / 64) * 4) * 512; }
// conv_f16x3v2.hip: the same arithmetic on v_mfma_f32_32x32x16_f16, 8 x 32-pixel tiles (bank layout 1)
bool f16x3v2_shape(int Ho, int Wo, int rows, int chans);      // layers it takes (whole tiles, 32-row fragments; which of them: measured, see the function): decides the bank layout
int f16x3v2_nf(int rows);
hipError_t launch_f16x3v2_weights_multi(const WinoJobs& jobs, hipStream_t st);      // the layout-1 jobs of a job table (row scales already made)
bool conv_f16x3v2_applicable(const ConvArgs& a);
hipError_t launch_conv_f16x3v2(const ConvArgs& a, hipStream_t st, bool four_wave = false);      // the 8-wave kernel; four_wave: tests / timing (force_cfg 605)
// conv_stem_f16x3.hip: the 7x7 / stride-2 ResNet stem on the fp16x3 arithmetic (one MFMA k-step per kernel row); a.wu = its bank
size_t stem_f16x3_bank_floats();
hipError_t launch_stem_f16x3_weights(const float* w, int Kpad, int cin_p, float* bank, hipStream_t st);
bool conv_stem_f16x3_applicable(const ConvArgs& a);
hipError_t launch_conv_stem_f16x3(const ConvArgs& a, hipStream_t st);
hipError_t launch_conv_f16x3(const ConvArgs& a, hipStream_t st, int variant = 0);      // variant: 0 auto | 1 four-wave kernel | 2 eight-wave kernel | 3 four-wave, 32-channel tiles (tests)
bool conv_wino_x3_applicable(const ConvArgs& a);
hipError_t launch_conv_wino_x3(const ConvArgs& a, hipStream_t st);
// process default (UWM_WINOGRAD / uwm_set_winograd): used by the single-operator entry points and by handles created later
bool winograd_enabled();
void winograd_set_mode(int mode);   // 0 off, 1 auto, 2 = tests: take the 8-wave variant wherever its shape rules allow
int winograd_mode();
// mode of ONE launch: the handle's own mode when its args carry one (wino = mode + 1), else the process default
static inline int wino_mode_of(int wino) { return wino > 0 ? wino - 1 : winograd_mode(); }

hipError_t launch_nchw_to_nhwc4(const float* x, float* y, int N, int C, int H, int W, int CP, hipStream_t st);
hipError_t launch_bn_finalize(const double* ssum, const double* ssq, const float* gamma, const float* beta,
                              float* run_mean, float* run_var, float* mean, float* rstd, float* scale, float* shift,
                              int C, double count, float eps, float momentum, int update_running, hipStream_t st,
                              int nrep = 1, int rep_stride = 0);
hipError_t launch_bn_eval(const float* gamma, const float* beta, const float* run_mean, const float* run_var,
                          float* scale, float* shift, int C, float eps, hipStream_t st);
// eval scale / shift of many BatchNorms in one launch (uwm_freeze).  Job: gamma at params + g_off, beta behind it; running mean at
// buffers + rm_off, running variance behind it; scale to out + out_off, shift behind it (C floats each).  Same arithmetic as launch_bn_eval.
struct BnEvalJob { unsigned g_off, rm_off, out_off; int C; float eps; };
struct BnEvalJobs { static constexpr int kMax = 128; BnEvalJob j[kMax]; int n; };
hipError_t launch_bn_eval_multi(const float* params, const float* buffers, float* out, const BnEvalJobs& jobs, hipStream_t st);
// xn = relu(y*s2+b2 + idn), idn = id (materialised) or id*sd+bd (lazy)
hipError_t launch_residual(const float* y, const float* s2, const float* b2, const float* id, const float* sd,
                           const float* bd, float* out, size_t npix, int C, hipStream_t st);
hipError_t launch_maxpool_fwd(const Src& in, float* out, uint8_t* idx, int N, int Ho, int Wo, hipStream_t st);
// g_in = (maxpool_bwd(g_out, idx) + addend) masked by relu(in.raw*scale+shift) > 0
hipError_t launch_maxpool_bwd(const float* gout, const uint8_t* idx, const float* addend, const Src& in, float* gin,
                              int N, int Ho, int Wo, hipStream_t st, const float* bn_mean = nullptr, const float* bn_rstd = nullptr,
                              double* ssum = nullptr, double* ssq = nullptr, int srep = 0, int sstride = 0);   // bn_*: fused BatchNorm-backward sums of the masked output
// BatchNorm backward: g = grad wrt BN output (already ReLU-masked), y = raw conv output
hipError_t launch_bn_bwd_reduce(const float* g, const float* y, const float* mean, const float* rstd,
                                double* dgamma, double* dbeta, size_t npix, int C, hipStream_t st);
hipError_t launch_bn_bwd_apply(const float* g, const float* y, const float* mean, const float* rstd,
                               const float* gamma, const double* dgamma, const double* dbeta, float* dy,
                               float* gamma_grad, float* beta_grad, size_t npix, int C, hipStream_t st,
                               const double* rep = nullptr, int nrep = 0, int rep_stride = 0, hipEvent_t done = nullptr,
                               float* xmax = nullptr);   // xmax: 32 zero-initialised floats; slot (workgroup & 31) receives max|dy| of the workgroup (ConvArgs::xmax of the fp16x3 dgrad that reads dy)   // rep: fold the nrep replicas {dbeta part[C], dgamma part[C]} of a fused dgrad epilogue in the prologue (dgamma / dbeta unused)
// dcat [N][H][W][C0+C1] -> gprev [N][H/2][W/2][C0] = mask(sum 2x2), gskip [N][H][W][C1] (copy)
hipError_t launch_upsplit(const float* dcat, int N, int H, int W, int C0, int C1, float* gprev,
                          const float* pmask, const float* pscale, const float* pshift, float* gskip,
                          hipStream_t st, int accumulate_prev = 0);
// UNet++ dense skips: materialise act(src) into a channel range of a concat buffer / scatter-accumulate a channel
// range of a concat gradient back (optionally ReLU-masked by the tensor it belongs to)
hipError_t launch_concat_copy(const Src& s, size_t npix, float* dst, int Cd, int dst_off, hipStream_t st);
hipError_t launch_split_accum(const float* gcat, int Cc, int off, int C, size_t npix, float* dst, const float* m,
                              const float* mscale, const float* mshift, int accumulate, hipStream_t st);
hipError_t launch_pack_dgrad(const float* w, int Cout, int Kpad, int ntaps, int Cin, float* wd, int KpadD,
                             int CoutP, hipStream_t st);
hipError_t launch_colsum(const float* g, size_t npix, int C, float* out, double* scratch, hipStream_t st);   // out[c] += sum over pixels; scratch (colsum_scratch_doubles(C)): two-stage, fixed order; nullptr: float atomics
size_t colsum_scratch_doubles(int C);
hipError_t launch_adam(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2,
                       float eps, float wd, float bc1, float bc2, float gscale, hipStream_t st,
                       const double* sumsq = nullptr, float max_norm = 0.f, bool decoupled = false);
hipError_t launch_adam_graph(float* p, const float* g, float* m, float* v, size_t n, float* hyp /* device, 10 floats */, const double* sumsq, hipStream_t st,
                             bool decoupled = false);      // decoupled: AdamW's weight decay
hipError_t launch_sumsq(const float* g, size_t n, double* out, hipStream_t st);
hipError_t launch_sgd(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float wd, int first, float gscale,
                      hipStream_t st, const double* sumsq = nullptr, float max_norm = 0.f);
hipError_t launch_resize_threshold(const float* logits, int ld, int N, int h, int w, int H, int W, float thr,
                                   int apply_sigmoid, uint8_t* out, float* out_f, hipStream_t st);
hipError_t launch_scale(float* p, size_t n, float s, hipStream_t st);
hipError_t launch_absmax32(const float* x, size_t n, float* out32, hipStream_t st);      // out32[0..31] <- max|x| (slot workgroup & 31; zeroed first): the xmax contract of the fp16x3 kernels
hipError_t launch_preprocess_u8(const uint8_t* img, int N, int H, int W, int C, const float* mean, const float* std,
                                const int* flags, float* out, hipStream_t st);
// uint8 [npix][C] (4-byte aligned) -> Normalize as fp32 [npix][4], padding channels zero: launch_preprocess_u8's values in the forward's input layout
hipError_t launch_preprocess_u8_nhwc4(const uint8_t* img, size_t npix, int C, const float* mean, const float* std, float* out,
                                      hipStream_t st);
hipError_t launch_preprocess_mask(const uint8_t* m, int N, int H, int W, int thr, const int* flags, uint8_t* out, hipStream_t st);
struct PreArgs { float mul[4], add[4]; };
// Normalize of one byte: ONE function (explicit fused multiply-add) for preprocess_u8_kernel, preprocess_u8_nhwc4_kernel and
// resize_norm_u8_nhwc4_kernel, so that the stem sees the same bits on every path
__device__ __forceinline__ float pre_norm(uint32_t b, float mul, float add) { return fmaf((float)b, mul, add); }
static inline PreArgs make_pre_args(int C, const float* mean, const float* std) {
  PreArgs pa;
  for (int c = 0; c < 4; ++c) { pa.mul[c] = 0.f; pa.add[c] = 0.f; }
  for (int c = 0; c < C; ++c) { pa.mul[c] = 1.f / (255.f * std[c]); pa.add[c] = -mean[c] / std[c]; }
  return pa;
}
// flags -> source index of uwm_preprocess_u8 / uwm_preprocess_mask_u8 / uwm_augment_u8: ONE function, so that the three agree
__device__ __forceinline__ void aug_src(int flags, int H, int W, int y, int x, int& sy, int& sx) {
  // output (y, x) of rot90^k(flip(img)) -> coordinates in the flipped image, then undo the flips
  const int k = (flags >> 2) & 3;
  int fy = y, fx = x;
  if (k == 1) { fy = x; fx = W - 1 - y; }            // torch.rot90(a, 1)[y][x] = a[x][W-1-y]
  else if (k == 2) { fy = H - 1 - y; fx = W - 1 - x; }
  else if (k == 3) { fy = H - 1 - x; fx = y; }
  if (flags & 1) fx = W - 1 - fx;
  if (flags & 2) fy = H - 1 - fy;
  sy = fy; sx = fx;
}
// ---- train-time augmentation (augment_u8.hip; the rule: include/uwm.h)
struct AugDesc { int flags, hue, sat, val; double minv[6]; unsigned char lut[256]; };      // = uwm_aug_desc: one per image, in DEVICE memory
// images [N][H][W][C] -> out_f fp32 NCHW (Normalize = pre_norm) and, where out_u8 != nullptr, the augmented bytes [N][H][W][C]
hipError_t launch_augment_u8(const uint8_t* img, const AugDesc* descs, int N, int H, int W, int C, const float* mean, const float* std,
                             float* out_f, uint8_t* out_u8, hipStream_t st);
// masks [N][H][W] -> nearest warp of the same descriptors, then (m > thr) as {0,1}
hipError_t launch_augment_mask(const uint8_t* m, const AugDesc* descs, int N, int H, int W, int thr, uint8_t* out, hipStream_t st);
// ---- the enhanced recipe's stages behind the basic ones (augment_ext_u8.hip; the rule: include/uwm.h)
struct AugExtDesc { int tone, clahe_clip, noise_sigma, blur; unsigned char blur_w[9]; unsigned long long seed; unsigned char lut2[256]; };   // = uwm_aug_ext_desc
size_t aug_ext_workspace_bytes(int N, int H, int W, int C);      // 0 for a bad shape
// ext == nullptr: launch_augment_u8 + launch_augment_mask as they are.  Otherwise the stage pass, the CLAHE tile tables and the apply pass.
hipError_t launch_augment_ext(const uint8_t* img, const uint8_t* masks, const AugDesc* descs, const AugExtDesc* ext, int N, int H, int W, int C,
                              const float* mean, const float* std, int thr, void* workspace, size_t workspace_bytes, float* out_f,
                              uint8_t* out_masks, uint8_t* out_u8, hipStream_t st);
bool aug_ext_host_table(int which, const void** data, int* count, int* elem_bytes);      // the host's tables (uwm_aug_lab_tables)
// ---- the transparent_watermark recipe's ImageCompression: a baseline 4:2:0 JPEG round trip (jpeg_u8.hip; the rule: include/uwm.h)
size_t jpeg_workspace_bytes(int N, int H, int W);      // 0 for a bad shape (H, W multiples of 16)
// images [N][H][W][3], quality DEVICE int[N] (0 = unchanged, else 1..100) -> out_f fp32 NCHW (Normalize = pre_norm) and / or the bytes out_u8
hipError_t launch_jpeg_u8(const uint8_t* img, const int* quality, int N, int H, int W, const float* mean, const float* std, void* workspace,
                          size_t workspace_bytes, float* out_f, uint8_t* out_u8, hipStream_t st);
// ---- the same round trip for a ragged batch, every image at its own size (jpeg_ragged_u8.hip; the edge rule: include/uwm.h)
struct ImageDesc;
constexpr int kJpegRaggedMaxBlocks = 512;              // most workgroups per image in either pass
constexpr long long kJpegRaggedPixelsPerBlock = 2048;  // K = ceil(max_pixels / this), 1 .. kJpegRaggedMaxBlocks: grid = N * K (measured)
int jpeg_ragged_blocks_per_image(long long max_pixels);
// image i of the packed batch (descs, quality: DEVICE memory; quality 0 = unchanged, else 1..100) -> out + descs[i].offset; out may be
// in.  The workspace holds `bytes` bytes.  No read leaves [in, in + bytes), no write [out, out + bytes) or the workspace
hipError_t launch_jpeg_ragged_u8(const uint8_t* in, uint8_t* out, size_t bytes, const ImageDesc* descs, const int* quality, int N,
                                 long long max_pixels, void* workspace, size_t workspace_bytes, hipStream_t st);
// One output pixel (Y, X) of the bilinear resize of a logit plane b[h][w] (element stride ld) by sy = h / H, sx = w / W: ONE function
// for resize_threshold_kernel (loss.hip) and resize_threshold_ragged_kernel (resize_u8.hip), so that a ragged batch's masks are the
// uniform call's bit for bit
__device__ __forceinline__ float resize_logit(const float* __restrict__ b, int ld, int h, int w, float sy, float sx, int Y, int X,
                                              int apply_sigmoid) {
  float fy = ((float)Y + 0.5f) * sy - 0.5f, fx = ((float)X + 0.5f) * sx - 0.5f;
  fy = fmaxf(fy, 0.f); fx = fmaxf(fx, 0.f);
  int y0 = (int)fy, x0 = (int)fx;
  y0 = min(y0, h - 1); x0 = min(x0, w - 1);
  const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
  const float wy = fy - (float)y0, wx = fx - (float)x0;
  const float v00 = b[((size_t)y0 * w + x0) * ld], v01 = b[((size_t)y0 * w + x1) * ld];
  const float v10 = b[((size_t)y1 * w + x0) * ld], v11 = b[((size_t)y1 * w + x1) * ld];
  float v = (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
  if (apply_sigmoid) v = 1.f / (1.f + expf(-v));
  return v;
}
// ---- cv2-convention resize of a ragged batch of uint8 images (resize_u8.hip; the rule: include/uwm.h)
constexpr int kResizeRowsPerBlock = 4;               // output rows of one resize workgroup: grid = N * ceil(H / this) (also the ABI's launch-size check)
struct ImageDesc { long long offset; int h, w; };      // = uwm_image_desc: one per image, in DEVICE memory
// [N] images (h_i, w_i, C) at src + offset_i -> uint8 [N][H][W][C]; interp 0 nearest | 1 linear.  No read leaves [src, src + src_bytes)
hipError_t launch_resize_u8(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int N, int C, int H, int W, int interp,
                            uint8_t* out, hipStream_t st);
// the linear resize, then Normalize (pre_norm) as fp32 [N][H][W][4], padding channels zero: launch_resize_u8 -> launch_preprocess_u8_nhwc4
hipError_t launch_resize_norm_u8_nhwc4(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int N, int C, int H, int W,
                                       const float* mean, const float* std, float* out, hipStream_t st);
// logit plane [N][h][w] (stride ld) -> image i's own (h_i, w_i) at mask + offset_i, thresholded; nothing is written outside [mask, mask + mask_bytes)
hipError_t launch_resize_threshold_ragged(const float* logits, int ld, int N, int h, int w, const ImageDesc* out_descs, float thr,
                                          int apply_sigmoid, uint8_t* mask, size_t mask_bytes, hipStream_t st);
// ---- prediction at native resolution: overlapping tiles, blended (tile_u8.hip; the rule: include/uwm.h)
constexpr int kTileRowsPerBlock = 4;                 // tile rows of one gather workgroup: grid = K * ceil(T_h / this)
constexpr int kTileBlendBlocks = 128;                // workgroups per image in the blend: grid = num_images * this
constexpr int kTileMaxSide = 1024;                   // the blend's integer weights and their sums are exact in float32 up to this tile side
struct TileDesc { int image, y0, x0, first; };       // = uwm_tile_desc: one per tile, in DEVICE memory
struct TileImage { int first, ny, nx, reserved; };   // = uwm_tile_image: one per image, in DEVICE memory
// tile k = (image, y0, x0) of the packed batch -> Normalize (pre_norm) as fp32 [K][T_h][T_w][4], reflect-101 where the tile leaves the
// image, zeros for an entry that does not check out.  No read leaves [src, src + src_bytes)
hipError_t launch_tile_norm_u8_nhwc4(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int num_images, const TileDesc* tiles, int K,
                                     int C, int T_h, int T_w, const float* mean, const float* std, float* out, hipStream_t st);
// channel 0 of logits [npix][ld] -> store [npix]
hipError_t launch_tile_store(const float* logits, int ld, size_t npix, float* store, hipStream_t st);
// store [K][T_h][T_w] -> image i's blended plane at its own size, thresholded into mask + out_descs[i].offset and, where logits_out !=
// nullptr, as floats at logits_out + out_descs[i].offset (mask_bytes floats).  in_descs (may be nullptr): the images the tiles were cut
// from; one that does not fit [0, src_bytes) gives a zero mask.  Nothing is written outside [mask, mask + mask_bytes)
hipError_t launch_tile_blend_threshold_ragged(const float* store, int K, const TileImage* plans, int num_images, int T_h, int T_w, int overlap,
                                              const ImageDesc* in_descs, size_t src_bytes, int C, const ImageDesc* out_descs, float thr,
                                              int apply_sigmoid, uint8_t* mask, size_t mask_bytes, float* logits_out, hipStream_t st);
// ---- test-time augmentation: the D4 views of the network input, merged on the way back (tta.hip; the rule: include/uwm.h)
// base planes a range of num_slots slots can touch at most: the staging buffer of the two calls below holds this many [H][W][4] planes (0: bad arguments)
int view_stage_planes(int views, int num_slots);
// slots [slot0, slot0 + num_slots) of the images (slot = image * k + j) -> out [num_slots][H][W][4]: launch_resize_norm_u8_nhwc4 of the
// images the range touches into `stage`, then the views; a slot whose image is >= num_images is written as zeros
hipError_t launch_resize_norm_view_u8_nhwc4(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int num_images, int C, int H, int W,
                                            const float* mean, const float* std, int views, int slot0, int num_slots, float* stage, float* out,
                                            hipStream_t st);
// the same for the tiles of a tile table of K entries (slot = tile * k + j): launch_tile_norm_u8_nhwc4 into `stage`, then the views
hipError_t launch_tile_norm_view_u8_nhwc4(const uint8_t* src, size_t src_bytes, const ImageDesc* descs, int num_images, const TileDesc* tiles, int K,
                                          int C, int T_h, int T_w, const float* mean, const float* std, int views, int slot0, int num_slots,
                                          float* stage, float* out, hipStream_t st);
// logit planes [num_slots][H][W] (stride ld) of that slot range, mapped back, into store [num_items][H][W]: first view writes, later add, last divides
hipError_t launch_view_merge(const float* logits, int ld, int H, int W, int views, int slot0, int num_slots, int num_items, float* store,
                             hipStream_t st);
// ---- masks from watermarked / clean pairs (pair_mask_u8.hip; the rule: include/uwm.h)
constexpr int kPairMaskBlocks = 64;                 // workgroups per image, each walking that image's tiles: grid = N * this
constexpr int kPairMaskTileW = 120, kPairMaskTileH = 32;      // mask pixels of one tile
// image i: mask + mask_descs[i].offset <- open3(gray(|wm_i - clean_i|) > threshold) (open == 0: without the opening); clean_descs[i].h == 0
// skips the image, any other misfit zeroes its mask.  No read leaves the two source buffers, no write leaves [mask, mask + mask_bytes)
hipError_t launch_pair_mask_u8(const uint8_t* wm, size_t wm_bytes, const ImageDesc* wm_descs, const uint8_t* clean, size_t clean_bytes,
                               const ImageDesc* clean_descs, int N, int threshold, int open, uint8_t* mask, size_t mask_bytes,
                               const ImageDesc* mask_descs, hipStream_t st);
// planes of byte pixels (0 / 255) in LDS, four to a dword, kPlaneGroups dwords to a row: what pair_mask_u8.hip and filter_u8.hip share
constexpr int kPlaneGroups = 32;
// bytes k = 0..3 of the result are 0xFF where 0 <= x + k < w
__device__ __forceinline__ uint32_t column_mask(int x, int w) {
  if (x >= 0 && x + 3 < w) return 0xFFFFFFFFu;
  uint32_t m = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) if (x + k >= 0 && x + k < w) m |= 0xFFu << (8 * k);
  return m;
}
// the cross (cv2's 3 x 3 ELLIPSE): centre, up, down, left, right of dword (r, g); AND = erosion, else dilation.  The columns left of
// group 0 and right of the last group read as 0, so each pass spoils one more plane column at either end: the halo covers them
template <bool AND>
__device__ __forceinline__ uint32_t cross(const uint32_t (*p)[kPlaneGroups], int r, int g) {
  const uint32_t c = p[r][g], up = p[r - 1][g], dn = p[r + 1][g];
  const uint32_t prev = g > 0 ? p[r][g - 1] : 0u, next = g < kPlaneGroups - 1 ? p[r][g + 1] : 0u;
  const uint32_t lf = (c << 8) | (prev >> 24), rt = (c >> 8) | (next << 24);
  return AND ? (c & up & dn & lf & rt) : (c | up | dn | lf | rt);
}
// four mask pixels (x .. x + 3 of row y) of an h x w mask at out: one dword where it is aligned and whole, else bytes
__device__ __forceinline__ void store_px4(uint8_t* __restrict__ out, int y, int x, int w, uint32_t v) {
  if (x >= w) return;
  uint8_t* p = out + (size_t)y * w + x;
  if (x + 3 < w && ((uintptr_t)p & 3) == 0) { *(uint32_t*)p = v; return; }
#pragma unroll
  for (int k = 0; k < 4; ++k) if (x + k < w) p[k] = (uint8_t)(v >> (8 * k));
}
// ---- the dataset filter: watermark area of every image of a ragged batch (filter_u8.hip; the rule: include/uwm.h)
constexpr int kFilterBlocks = 64;                    // workgroups per image, each walking that image's tiles: grid = N * this
constexpr int kFilterTileW = 120, kFilterTileH = 32; // mask pixels of one tile
// One output pixel (Y, X) in watermark_filter.py's order: the sigmoid (loss.hip's form) at the four taps FIRST, then resize_logit's
// interpolation on the four probabilities, with its coordinates, clamps and order of operations
__device__ __forceinline__ float resize_prob(const float* __restrict__ b, int ld, int h, int w, float sy, float sx, int Y, int X) {
  float fy = ((float)Y + 0.5f) * sy - 0.5f, fx = ((float)X + 0.5f) * sx - 0.5f;
  fy = fmaxf(fy, 0.f); fx = fmaxf(fx, 0.f);
  int y0 = (int)fy, x0 = (int)fx;
  y0 = min(y0, h - 1); x0 = min(x0, w - 1);
  const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
  const float wy = fy - (float)y0, wx = fx - (float)x0;
  const float v00 = 1.f / (1.f + expf(-b[((size_t)y0 * w + x0) * ld])), v01 = 1.f / (1.f + expf(-b[((size_t)y0 * w + x1) * ld]));
  const float v10 = 1.f / (1.f + expf(-b[((size_t)y1 * w + x0) * ld])), v11 = 1.f / (1.f + expf(-b[((size_t)y1 * w + x1) * ld]));
  return (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
}
size_t filter_workspace_bytes(int N);                // 0 for N < 1 or a launch too large
// image i: counts[i] = {foreground pixels, h_i * w_i} of close3(open3(resize(sigmoid(logits_i)) > thr)) (post_process == 0: without
// the morphology) and, where mask != nullptr, that mask at mask + out_descs[i].offset.  A misfit image counts {0, 0}.  No write
// leaves [mask, mask + mask_bytes), counts[0 .. 2N) or the workspace
hipError_t launch_prob_mask_count(const float* logits, int ld, int N, int h, int w, const ImageDesc* out_descs, float thr, int post_process,
                                  uint8_t* mask, size_t mask_bytes, long long* counts, void* workspace, size_t workspace_bytes,
                                  hipStream_t st);
// ---- logo-watermarked training samples (synth_u8.hip; the rule: include/uwm.h)
constexpr int kSynthBlocks = 32;                     // workgroups per job in every stage launch: grid = N * K * this
constexpr int kSynthMaxSlots = 8;                    // K, the logo slots of one image
constexpr long long kSynthMaxPatchPixels = 1ll << 26, kSynthMaxTaps = 1ll << 24;
struct SynthJob {                                    // = uwm_synth_job: one per (image, slot), in DEVICE memory
  int enabled, logo, w1, h1, rotate, w2, h2, stretch, w3, h3, shear, blur, blur_r;
  unsigned blur_ww, blur_fw;
  int ndefects, defects[3][4], enhance;
  float brightness, contrast, color;
  int x, y;
  double rot[6], shear_minv[6];
  uint8_t opacity[256];
};
size_t synth_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps);      // 0 for arguments out of range
int synth_lanczos_ksize(int in, int out);            // taps per output of the table in -> out (host)
// int32 [out][2 + ksize] = {xmin, xmax, coefficients} of Pillow's LANCZOS resample in -> out, built in fp64 on the device
hipError_t launch_lanczos_table(int in, int out, int* table, hipStream_t st);
// stages 1-8 of every job, in place on the ragged RGB batch; masks (may be nullptr) <- the pasted alpha planes.  No read leaves the
// inputs, no write leaves [images, +image_bytes), [masks, +mask_bytes) or the workspace
hipError_t launch_synth_u8(uint8_t* images, size_t image_bytes, const ImageDesc* image_descs, uint8_t* masks, size_t mask_bytes,
                           const ImageDesc* mask_descs, const uint8_t* logos, size_t logo_bytes, const ImageDesc* logo_descs, int num_logos,
                           const SynthJob* jobs, int N, int K, long long max_patch_pixels, long long max_taps, void* ws, size_t ws_bytes,
                           hipStream_t st);
// stages 1-7 only: job j's finished RGBA patch -> out + j * max_patch_pixels * 4 (a job that is off or does not fit writes nothing)
hipError_t launch_synth_patches(const uint8_t* logos, size_t logo_bytes, const ImageDesc* logo_descs, int num_logos, const SynthJob* jobs, int J,
                                long long max_patch_pixels, long long max_taps, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes,
                                hipStream_t st);
// ---- text-watermarked training samples (synth_text_u8.hip; the rule: include/uwm.h).  K, the workgroups per job and the
// capacities are the logo chain's
struct TextJob {                                     // = uwm_text_job: one per (image, slot), in DEVICE memory
  int enabled, glyph, ink[3], rotate, w2, h2, scale, w3, h3, blur, blur_r;
  unsigned blur_ww, blur_fw;
  int brighten, recontrast;
  float brightness, contrast;
  int nfit, fit[3][2], x, y;
  double rot[6];
  uint8_t opacity[256];
};
size_t synth_text_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps);      // 0 for arguments out of range
// stages A-H of every job, in place on the ragged RGB batch; masks (may be nullptr) follow mask_mode (0: paste over the plane, 1: the
// mixed rule).  No read leaves the inputs, no write leaves [images, +image_bytes), [masks, +mask_bytes) or the workspace
hipError_t launch_synth_text_u8(uint8_t* images, size_t image_bytes, const ImageDesc* image_descs, uint8_t* masks, size_t mask_bytes,
                                const ImageDesc* mask_descs, int mask_mode, const uint8_t* planes, size_t plane_bytes,
                                const ImageDesc* plane_descs, int num_planes, const TextJob* jobs, int N, int K, long long max_patch_pixels,
                                long long max_taps, void* ws, size_t ws_bytes, hipStream_t st);
// stages A-G only: job j's finished RGBA patch -> out + j * max_patch_pixels * 4 (a job that is off or does not fit writes nothing)
hipError_t launch_text_patches(const uint8_t* planes, size_t plane_bytes, const ImageDesc* plane_descs, int num_planes, const TextJob* jobs, int J,
                               long long max_patch_pixels, long long max_taps, void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes,
                               hipStream_t st);

// EfficientNet MBConv pieces (mbconv.hip): swish, depthwise k x k conv (weights tap-major [k*k][C]) with static "same"
// padding (pb = pad at the begin of H and W; the end pad is implied by Ho/Wo), squeeze-and-excitation, block output with drop-connect
hipError_t launch_swish_fwd(const float* y, const float* sc, const float* sh, int C, float* out, size_t npix, hipStream_t st);
hipError_t launch_dw_fwd(const float* x, const float* w, int k, int stride, int pb, int N, int H, int W, int C,
                         int Ho, int Wo, float* y, hipStream_t st);
hipError_t launch_dw_dgrad(const float* dy, const float* w, int k, int stride, int pb, int N, int H, int W, int C,
                           int Ho, int Wo, const float* addend, float* dx, hipStream_t st);
// two-stage (partials + reduce, no global atomics): scratch holds dw_wgrad_scratch_floats(...) floats; dw += result
size_t dw_wgrad_scratch_floats(int k, int N, int C, int Ho, int Wo);
hipError_t launch_dw_wgrad(const float* x, const float* dy, int k, int stride, int pb, int N, int H, int W, int C,
                           int Ho, int Wo, float* dw, float* scratch, hipStream_t st);
// BatchNorm backward behind swish [and the SE product]: swish_bwd fused into both BatchNorm-backward passes
hipError_t launch_bn_bwd_act(const float* g, const float* y, const float* mean, const float* rstd, const float* gamma, const float* scale,
                             const float* shift, const float* se_s, const float* gpool, int N, size_t hw, double* dgamma, double* dbeta,
                             float* dy, float* gamma_grad, float* beta_grad, int C, hipStream_t st,
                             float* xmax = nullptr);   // xmax: as launch_bn_bwd_apply's (32 zero-initialised floats <- max|dy|)
hipError_t launch_colstats(const float* y, size_t npix, int C, double* ssum, double* ssq, hipStream_t st);
// out[n][c] = scale * sum_hw a[n][hw][c] (* b[n][hw][c]); deterministic two-stage sum, part: se_reduce_scratch_floats(N, C) floats
size_t se_reduce_scratch_floats(int N, int C);
hipError_t launch_se_reduce_hw(const float* a, const float* b, int N, size_t hw, int C, float scale, float* out, float* part, hipStream_t st);
hipError_t launch_swish_pool(const float* y, const float* sc, const float* sh, float* act_out, int N, size_t hw, int C, float* pool,
                             float* part, hipStream_t st);
hipError_t launch_se_fc_fwd(const float* pool, const float* w1, const float* b1, int K1pad, const float* w2, const float* b2,
                            int K2pad, int N, int C, int nsq, float* hpre, float* hid /* scratch [N][nsq] */, float* s, hipStream_t st);
// gs [N][C] is overwritten (gz2); acc1: scratch [N][nsq] zeroed by the caller; parameter gradients are plain stores
hipError_t launch_se_fc_bwd(float* gs, const float* s, const float* hpre, const float* pool, const float* w1, int K1pad,
                            const float* w2, int K2pad, int N, int C, int nsq, float* gpool, float* acc1, float* gw1,
                            float* gb1, float* gw2, float* gb2, hipStream_t st);
hipError_t launch_se_scale(const float* a, const float* s, int N, size_t hw, int C, float* out, hipStream_t st);
// out = (y*sc+sh) * rowscale[n] + id   (rowscale / id may be nullptr)
hipError_t launch_mb_out(const float* y, const float* sc, const float* sh, const float* rowscale, const float* id, int N, size_t hw,
                         int C, float* out, hipStream_t st);
hipError_t launch_rowscale(const float* g, const float* rowscale, int N, size_t hw, int C, float* out, hipStream_t st);

// loss / metrics (loss.hip)
hipError_t launch_loss(const float* logits, int ld, const void* target, int tdtype, size_t npix_total,
                       float w_dice, float w_bce, float smooth, float eps, double* scratch4, float* loss_out3,
                       float* dlogits, int ldd, float grad_scale, hipStream_t st);
hipError_t launch_loss_sums(const float* logits, int ld, const void* target, int tdtype, size_t n, double* scratch4, hipStream_t st);
hipError_t launch_loss_apply(const float* logits, int ld, const void* target, int tdtype, size_t n, double ntotal, float w_dice, float w_bce,
                             float smooth, float eps, const double* scratch4, float* loss_out3, float* dlogits, int ldd,
                             float grad_scale, hipStream_t st);
// Dice + BCE + Jaccard + Tversky + Focal (loss_ext.hip); scratch: 64 bytes (5 doubles in use, all 8 zeroed), loss_out8: 8 floats
hipError_t launch_loss_ext(const float* logits, int ld, const void* target, int tdtype, size_t n, const uwm_loss_spec& spec,
                           double* scratch, float* loss_out8, float* dlogits, int ldd, float grad_scale, hipStream_t st);
hipError_t launch_loss_ext_sums(const float* logits, int ld, const void* target, int tdtype, size_t n, const uwm_loss_spec& spec,
                                double* scratch, hipStream_t st);
hipError_t launch_loss_ext_apply(const float* logits, int ld, const void* target, int tdtype, size_t n, double ntotal,
                                 const uwm_loss_spec& spec, const double* scratch, float* loss_out8, float* dlogits, int ldd,
                                 float grad_scale, hipStream_t st);
hipError_t launch_stats(const float* logits, int ld, const void* target, int tdtype, int N, size_t hw,
                        float thr, int apply_sigmoid, long long* out4, hipStream_t st);
hipError_t launch_threshold(const float* logits, int ld, size_t npix, float thr, int apply_sigmoid,
                            uint8_t* out, hipStream_t st);

// mask post-processing (mask_post.hip): the reference's _optimize_mask on bit planes + union-find components.  ws holds
// mask_workspace_bytes(N, H, W) bytes; the callers (uwm_abi.inc) have checked every argument
int mask_element(int shape, int kw, int kh, uint8_t* out);      // host: kh*kw bytes of 0/1; non-zero on a bad shape / size
size_t mask_workspace_bytes(int N, int H, int W);
hipError_t launch_mask_morph(const uint8_t* in, uint8_t* out, int N, int H, int W, int dilate, int shape, int kw, int kh,
                             int iterations, void* ws, hipStream_t st);
hipError_t launch_mask_components(const uint8_t* in, int* labels, int* areas, int N, int H, int W, void* ws, hipStream_t st);
hipError_t launch_optimize_mask(const uint8_t* in, uint8_t* out, int N, int H, int W, int mask_type, long long* summary, void* ws,
                                hipStream_t st);
// the same on a ragged batch (image i: descs[i], read on the device); mask_type 3 = no morphology, every component kept.
// ws: mask_ragged_workspace_bytes(N, mask_bytes, rows) bytes; stats (may be null): [N][8], include/uwm.h
size_t mask_ragged_workspace_bytes(int N, size_t mask_bytes, long long rows);
hipError_t launch_optimize_masks_ragged(const uint8_t* in, uint8_t* out, size_t mask_bytes, const ImageDesc* descs, int N, int mask_type,
                                        long long max_pixels, long long rows, long long* stats, void* ws, hipStream_t st);
// region and Boundary-IoU counts of a ragged batch of mask pairs (mask_score.hip; the rule: include/uwm.h).
// descs, radius: DEVICE memory; counts: [N][8]; ws: score_masks_workspace_bytes(N, mask_bytes, rows) bytes
size_t score_masks_workspace_bytes(int N, size_t mask_bytes, long long rows);
hipError_t launch_score_masks_ragged(const uint8_t* pred, const uint8_t* truth, size_t mask_bytes, const ImageDesc* descs, const int* radius,
                                     int N, long long max_pixels, long long rows, long long* counts, void* ws, hipStream_t st);
// exact squared Euclidean distance transforms of a ragged batch and the surface distances of mask pairs (mask_dist.hip; the rule:
// include/uwm.h).  descs: DEVICE memory; d2: [mask_bytes] int32; records: [N][10]; sums: [N][2]
size_t edt_workspace_bytes(int N, size_t mask_bytes, long long rows);
hipError_t launch_edt_ragged(const uint8_t* masks, size_t mask_bytes, const ImageDesc* descs, int N, long long max_pixels, long long rows,
                             int* d2, void* ws, hipStream_t st);
size_t surface_distances_workspace_bytes(int N, size_t mask_bytes, long long rows);
hipError_t launch_surface_distances_ragged(const uint8_t* pred, const uint8_t* truth, size_t mask_bytes, const ImageDesc* descs, int N,
                                           long long max_pixels, long long rows, long long* records, double* sums, void* ws, hipStream_t st);

// mask enhancement (mask_enhance.hip): the reference's enhance_mask on a ragged batch, grey morphology + float blur + binary
// smoothing (the rule: include/uwm.h).  ws: enhance_workspace_bytes(N, mask_bytes) bytes; stats (may be null): [N][4]
int enhance_gauss_taps(int blur_kernel, float* out);           // host: the taps (0..63; even + 1) -> their number, 0 on a bad argument
size_t enhance_workspace_bytes(int N, size_t mask_bytes);
hipError_t launch_enhance_masks_ragged(const uint8_t* in, uint8_t* out, size_t mask_bytes, const ImageDesc* descs, int N, int expand_pixels,
                                       int blur_kernel, int smooth_iterations, long long max_pixels, long long* stats, void* ws,
                                       hipStream_t st);

// watermark cut-outs from watermarked / clean pairs (extract_u8.hip): the reference's extract_watermarks.py on a ragged batch (the rule:
// include/uwm.h).  ws: extract_workspace_bytes(N, total_pixels, J) bytes, the larger of the two stages' needs (N or J
// below 1: that stage is left out); the callers (uwm_abi.inc) have checked every argument
constexpr int kExtractMaxRegions = 254;              // kept regions of one image: the plane's byte 255 stands for "none"
constexpr int kExtractRowInts = 9;                   // a table row: id, a00, a10, a01, x0, y0, x1, y1, pixels
struct ExtractJob {                                  // = uwm_extract_job: one cut-out, in DEVICE memory
  int image, x, y, w, h, reserved;
  long long out_offset;
  uint8_t member[256];
};
size_t extract_workspace_bytes(int N, long long total_pixels, int J);
// stage 1: stats [N][4] = {regions found, regions kept, status, h*w}, table [N][254][9], plane + plane_descs[i].offset <- the index
// of the kept region at each pixel or 255.  No read leaves the inputs, no write leaves the plane, stats, table or the workspace
hipError_t launch_extract_regions(const uint8_t* wm, size_t wm_bytes, const ImageDesc* wm_descs, const uint8_t* clean, size_t clean_bytes,
                                  const ImageDesc* clean_descs, int N, int threshold, int min_area, long long max_pixels, long long total_pixels,
                                  uint8_t* plane, size_t plane_bytes, const ImageDesc* plane_descs, long long* stats, long long* table, void* ws,
                                  hipStream_t st);
// stage 2: job j's enhanced RGBA crop -> out + jobs[j].out_offset, status[j] = 0 done | 1 misfit (nothing written)
hipError_t launch_extract_cutouts(const uint8_t* wm, size_t wm_bytes, const ImageDesc* wm_descs, const uint8_t* plane, size_t plane_bytes,
                                  const ImageDesc* plane_descs, int N, const ExtractJob* jobs, int J, long long max_crop_pixels, uint8_t* out,
                                  size_t out_bytes, int* status, void* ws, hipStream_t st);

// text-feature enhancement (text_enhance.hip): the reference's _enhance_text_features on a ragged batch of RGB images (the rule:
// include/uwm.h).  ws: text_enhance_workspace_bytes(total_pixels, N) bytes, its first N ints the per-image status;
// edges (may be null): the dilated edge plane.  The callers (uwm_abi.inc) have checked every argument
size_t text_enhance_workspace_bytes(long long total_pixels, int N);
hipError_t launch_text_enhance_ragged(const uint8_t* in, uint8_t* out, size_t bytes, const ImageDesc* descs, int N, long long max_pixels,
                                      long long total_pixels, uint8_t* edges, size_t edges_bytes, const ImageDesc* edge_descs, void* ws,
                                      hipStream_t st);

// membrane fill of the hole pixels of a ragged batch (inpaint.hip): pull-push, then `cycles` multigrid V-cycles on the hole (the
// rule: include/uwm.h).  ws: inpaint_workspace_bytes(N, image_bytes, C, max_side) bytes; stats (may be null): [N][4].
// The callers (uwm_abi.inc) have checked every argument
size_t inpaint_workspace_bytes(int N, size_t image_bytes, int C, int max_side);
int inpaint_launch_count(int cycles, int max_side);
hipError_t launch_inpaint_ragged(const uint8_t* images, uint8_t* out, size_t image_bytes, const ImageDesc* img_descs, const uint8_t* masks,
                                 size_t mask_bytes, const ImageDesc* mask_descs, int N, int C, int cycles, long long max_pixels, long long rows,
                                 int max_side, long long* stats, void* ws, hipStream_t st);

}  // namespace uwm
