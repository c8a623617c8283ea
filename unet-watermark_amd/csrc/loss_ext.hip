// The rest of the reference's loss menu on one fused pass: Dice + BCE-with-logits + Jaccard + Tversky + Focal, any weighted mix,
// for gfx950.  Same two halves as loss.hip: one read of logits/targets leaves the batch sums {sum p*t, sum p, sum t, sum bce,
// sum focal} in fp64 (wavefront, then workgroup, then one atomic per workgroup and sum); a second elementwise pass writes
// grad_scale * dL/dlogits from coefficients formed in fp64 from those sums.  loss.hip and its entry points are untouched: a
// Dice / BCE-only caller keeps using them.
//
// Reference semantics replaced (get_loss_function of the reference's src/utils/losses.py:20-27), all in mode='binary',
// from_logits=True, with smp's defaults for what that function does not pass:
//   smp.losses.JaccardLoss(smooth, eps=1e-7)                      1 - (I+smooth) / max(P+T-I+smooth, eps)
//   smp.losses.TverskyLoss(smooth, eps, alpha, beta, gamma)       (1 - (I+smooth) / max(I+alpha(P-I)+beta(T-I)+smooth, eps)) ^ gamma
//   smp.losses.FocalLoss(alpha=None, gamma=2, reduction='mean')   mean a_i (1-pt_i)^gamma bce_i,  pt_i = exp(-bce_i)
// with I = sum p*t, P = sum p, T = sum t; the region losses are 0 when T == 0 (smp's mask of empty classes).
//
// Every region loss has a gradient of the form s_i (ct*t_i + c0), s_i = p_i (1-p_i), so one pair (ct, c0) carries the weighted
// sum of Dice, Jaccard and Tversky and a Jaccard or Tversky run does the per-pixel arithmetic of a Dice run.  The focal
// arithmetic (expm1f, powf, a division) is a template parameter, compiled out when w_focal == 0.
#include "../../include/uwm.h"
#include "uwm_kernels.h"

namespace uwm {
namespace {

// target dtypes: 0 = float32, 1 = int64, 2 = uint8, 3 = int32
__device__ __forceinline__ float ext_target(const void* t, int dt, size_t i) {
  switch (dt) {
    case 0: return ((const float*)t)[i];
    case 1: return (float)((const long long*)t)[i];
    case 2: return (float)((const unsigned char*)t)[i];
    default: return (float)((const int*)t)[i];
  }
}

__device__ __forceinline__ double ext_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// a_i of the focal loss: alpha*t + (1-alpha)(1-t), or 1 without alpha (fa < 0)
__device__ __forceinline__ float focal_weight(float fa, float t) { return fa >= 0.f ? fa * t + (1.f - fa) * (1.f - t) : 1.f; }

// scratch: [0]=sum p*t [1]=sum p [2]=sum t [3]=sum bce [4]=sum focal (left at 0 when !FOCAL)
template <bool FOCAL>
__global__ __launch_bounds__(256) void loss_ext_reduce_kernel(const float* __restrict__ logits, int ld, const void* __restrict__ target,
                                                              int tdtype, size_t n, float fa, float fg, double* scratch) {
  float s_pt = 0.f, s_p = 0.f, s_t = 0.f, s_b = 0.f, s_f = 0.f;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float x = logits[i * ld];
    const float t = ext_target(target, tdtype, i);
    const float sp = log1pf(expf(-fabsf(x)));        // softplus(-|x|)
    const float p = expf(fminf(x, 0.f) - sp);        // exp(logsigmoid(x))
    const float bce = fmaxf(x, 0.f) - x * t + sp;
    s_pt += p * t; s_p += p; s_t += t;
    s_b += bce;
    if constexpr (FOCAL) {
      const float om = fmaxf(-expm1f(-bce), 0.f);    // 1 - pt without the cancellation at confident pixels
      s_f += focal_weight(fa, t) * powf(om, fg) * bce;
    }
  }
  constexpr int NS = FOCAL ? 5 : 4;
  __shared__ double red[4][NS];
  double v[NS] = {(double)s_pt, (double)s_p, (double)s_t, (double)s_b};
  if constexpr (FOCAL) v[NS - 1] = (double)s_f;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double w = ext_wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) red[wave][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const double s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    atomicAdd(scratch + threadIdx.x, s);
  }
}

// The loss terms and the gradient's coefficients from the sums, in fp64.  dL/dx_i = s_i (ct*t_i + c0) + wb (p_i - t_i)
// + wf * [focal factor of pixel i]; grad_scale is folded into all four.  A term whose weight is 0 adds no arithmetic to the
// coefficients (the elementwise pass forms them in every thread); `terms` asks for the loss values as well (the finalize thread).
struct ExtCoef { float ct, c0, wb, wf; double ldice, lbce, ljac, ltv, lfocal; };
__device__ __forceinline__ ExtCoef ext_coef(const double* s, double n, const uwm_loss_spec& q, double gscale, bool terms) {
  ExtCoef c;
  const double I = s[0], P = s[1], T = s[2];
  const bool on = T > 0.0;                       // smp masks the region losses of a batch without foreground
  double ct = 0.0, c0 = 0.0;
  c.ldice = c.ljac = c.ltv = 0.0;
  if (terms || q.w_dice != 0.f) {
    // d(1-score)/dx_i = -(A*t_i - B) s_i; the clamp kills the denominator's derivative (as loss.hip)
    const double sm = (double)q.dice_smooth, eps = (double)q.dice_eps, den = P + T + sm, denc = den > eps ? den : eps;
    c.ldice = on ? 1.0 - (2.0 * I + sm) / denc : 0.0;
    if (on) { ct -= (double)q.w_dice * (2.0 / denc); c0 += (double)q.w_dice * (den > eps ? (2.0 * I + sm) / (denc * denc) : 0.0); }
  }
  if (terms || q.w_jaccard != 0.f) {
    // score = (I+sm)/den, den = P+T-I+sm: dscore_i = s_i (A t_i - B (1-t_i)), A = 1/den, B = (I+sm)/den^2
    const double sm = (double)q.jaccard_smooth, eps = (double)q.jaccard_eps, den = P + T - I + sm, denc = den > eps ? den : eps;
    c.ljac = on ? 1.0 - (I + sm) / denc : 0.0;
    if (on) {
      const double A = 1.0 / denc, B = den > eps ? (I + sm) / (denc * denc) : 0.0;
      ct -= (double)q.w_jaccard * (A + B); c0 += (double)q.w_jaccard * B;
    }
  }
  if (terms || q.w_tversky != 0.f) {
    // den = I + a(P-I) + b(T-I) + sm: dden_i = s_i (t_i + a(1-t_i) - b t_i); loss = (1-score)^g
    const double sm = (double)q.tversky_smooth, eps = (double)q.tversky_eps, a = (double)q.tversky_alpha, b = (double)q.tversky_beta;
    const double g = (double)q.tversky_gamma;
    const double den = I + a * (P - I) + b * (T - I) + sm, denc = den > eps ? den : eps;
    double base = on ? 1.0 - (I + sm) / denc : 0.0;
    if (base < 0.0) base = 0.0;                  // (score > 1 only by rounding; a negative base has no real power)
    c.ltv = g == 1.0 ? base : pow(base, g);
    // g (1-score)^(g-1); at score == 1 the derivative of a g < 1 power is unbounded and is left out (0) instead of inf
    const double K = g == 1.0 ? (on ? 1.0 : 0.0) : (base > 0.0 ? g * pow(base, g - 1.0) : 0.0);
    const double A = 1.0 / denc, B = den > eps ? (I + sm) / (denc * denc) : 0.0;
    ct -= (double)q.w_tversky * K * (A - B * (1.0 - a - b)); c0 += (double)q.w_tversky * K * B * a;
  }
  c.lbce = s[3] / n;
  c.lfocal = q.w_focal != 0.f ? s[4] / n : 0.0;
  c.ct = (float)(gscale * ct); c.c0 = (float)(gscale * c0);
  c.wb = (float)(gscale * (double)q.w_bce / n); c.wf = (float)(gscale * (double)q.w_focal / n);
  return c;
}

__global__ void loss_ext_finalize_kernel(const double* scratch, double n, uwm_loss_spec q, float* out8) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const ExtCoef c = ext_coef(scratch, n, q, 1.0, true);
    out8[0] = (float)((double)q.w_dice * c.ldice + (double)q.w_bce * c.lbce + (double)q.w_jaccard * c.ljac +
                      (double)q.w_tversky * c.ltv + (double)q.w_focal * c.lfocal);
    out8[1] = (float)c.ldice; out8[2] = (float)c.lbce; out8[3] = (float)c.ljac; out8[4] = (float)c.ltv; out8[5] = (float)c.lfocal;
    out8[6] = 0.f; out8[7] = 0.f;
  }
}

// V4: ldd == 4 and a 16-byte aligned dlogits: gradient and its three zero padding channels leave as one 16-byte store
template <bool FOCAL, bool V4>
__global__ __launch_bounds__(256) void loss_ext_grad_kernel(const float* __restrict__ logits, int ld, const void* __restrict__ target,
                                                            int tdtype, size_t n, double ntotal, const double* scratch, uwm_loss_spec q,
                                                            float* __restrict__ dlogits, int ldd, float gscale) {
  // ntotal: pixels behind the sums in `scratch` (== n unless the sums were all-reduced over data-parallel ranks)
  const ExtCoef c = ext_coef(scratch, ntotal, q, (double)gscale, false);
  const float ct = c.ct, c0 = c.c0, wb = c.wb, wf = c.wf, fa = q.focal_alpha, fg = q.focal_gamma;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float x = logits[i * ld];
    const float t = ext_target(target, tdtype, i);
    const float sp = log1pf(expf(-fabsf(x)));
    const float p = expf(fminf(x, 0.f) - sp);
    float g = p * (1.f - p) * (ct * t + c0) + wb * (p - t);
    if constexpr (FOCAL) {
      // d[(1-pt)^g bce]/dx = (p-t) (1-pt)^(g-1) (g pt bce + (1-pt)) = (p-t) (1-pt)^g (g pt r + 1), r = bce/(1-pt) -> 1 as
      // 1-pt -> 0: no negative power, so g < 1 stays finite at confident pixels
      const float bce = fmaxf(x, 0.f) - x * t + sp;
      const float om = fmaxf(-expm1f(-bce), 0.f);
      const float pt = expf(-bce);
      const float r = om > 0.f ? bce / om : 1.f;
      g += wf * focal_weight(fa, t) * (p - t) * powf(om, fg) * (fg * pt * r + 1.f);
    }
    if constexpr (V4) {
      *reinterpret_cast<float4*>(dlogits + i * 4) = make_float4(g, 0.f, 0.f, 0.f);
    } else {
      float* o = dlogits + i * ldd;
      o[0] = g;
      for (int k = 1; k < ldd; ++k) o[k] = 0.f;
    }
  }
}

unsigned loss_ext_blocks(size_t n) { size_t nb = (n + 1023) / 1024; if (nb > 2048) nb = 2048; if (nb < 1) nb = 1; return (unsigned)nb; }

}  // namespace

// first half: scratch[0..4] = local {sum p*t, sum p, sum t, sum bce, sum focal}
hipError_t launch_loss_ext_sums(const float* logits, int ld, const void* target, int tdtype, size_t n, const uwm_loss_spec& q,
                                double* scratch, hipStream_t st) {
  // the whole 64-byte scratch block, not the 40 bytes in use: the runtime splits a fill that is no multiple of 16 bytes into two
  // fill kernels (measured: +3 us per call at 16 x 512 x 512)
  hipError_t e = hipMemsetAsync(scratch, 0, 8 * sizeof(double), st);
  if (e != hipSuccess) return e;
  const dim3 grid(loss_ext_blocks(n)), block(256);
  if (q.w_focal != 0.f)
    hipLaunchKernelGGL(loss_ext_reduce_kernel<true>, grid, block, 0, st, logits, ld, target, tdtype, n, q.focal_alpha, q.focal_gamma, scratch);
  else
    hipLaunchKernelGGL(loss_ext_reduce_kernel<false>, grid, block, 0, st, logits, ld, target, tdtype, n, q.focal_alpha, q.focal_gamma, scratch);
  return hipGetLastError();
}

// second half: the eight loss terms and dL/dlogits from the sums in scratch, which cover ntotal pixels (>= n when all-reduced)
hipError_t launch_loss_ext_apply(const float* logits, int ld, const void* target, int tdtype, size_t n, double ntotal,
                                 const uwm_loss_spec& q, const double* scratch, float* loss_out8, float* dlogits, int ldd,
                                 float grad_scale, hipStream_t st) {
  hipLaunchKernelGGL(loss_ext_finalize_kernel, dim3(1), dim3(64), 0, st, scratch, ntotal, q, loss_out8);
  if (dlogits) {
    const dim3 grid(loss_ext_blocks(n)), block(256);
    const bool focal = q.w_focal != 0.f, v4 = ldd == 4 && ((uintptr_t)dlogits & 15) == 0;
#define UWM_EXT_GRAD(F, V) hipLaunchKernelGGL((loss_ext_grad_kernel<F, V>), grid, block, 0, st, logits, ld, target, tdtype, n, ntotal, \
                                              scratch, q, dlogits, ldd, grad_scale)
    if (focal) { if (v4) UWM_EXT_GRAD(true, true); else UWM_EXT_GRAD(true, false); }
    else { if (v4) UWM_EXT_GRAD(false, true); else UWM_EXT_GRAD(false, false); }
#undef UWM_EXT_GRAD
  }
  return hipGetLastError();
}

hipError_t launch_loss_ext(const float* logits, int ld, const void* target, int tdtype, size_t n, const uwm_loss_spec& q,
                           double* scratch, float* loss_out8, float* dlogits, int ldd, float grad_scale, hipStream_t st) {
  hipError_t e = launch_loss_ext_sums(logits, ld, target, tdtype, n, q, scratch, st);
  if (e != hipSuccess) return e;
  return launch_loss_ext_apply(logits, ld, target, tdtype, n, (double)n, q, scratch, loss_out8, dlogits, ldd, grad_scale, st);
}

}  // namespace uwm
