// Per-element arithmetic the gradient-guided transfer shares between translation units:
//   guidance_push   : x - scale * (g_direct + g_unet)                    (guidance_apply_kernel, guided_step_kernel)
//   lp_x0, lp_reduce_body, lp_grad_body : the two passes of pd_lp_guidance (train_kernels.hip) and of pd_lp_guidance_scaled
//                                                                        (guided_kernels.hip)
// One definition each, so a fused kernel rounds exactly like the launches it replaces.  The scheduler update itself (ddim_step_elem and
// its halves, guidance_combine, the quad walker) lives in pd_step.h, included here.
#pragma once
#include "pd_step.h"

namespace pd {

// images - guidance_loss_scale * guidance_grad (utils_Img2Img.py:747-751).  The sum rounds once, then ONE fused multiply-add: the form
// the compiler gave guidance_apply_kernel's `x - s * (gd + gu)`, spelled out so that every caller gets it whatever surrounds the call.
__device__ __forceinline__ float guidance_push(float x, float s, float g_direct, float g_unet) {
#pragma clang fp contract(off)
  const float g = g_direct + g_unet;
  return __builtin_fmaf(-s, g, x);
}

// ---- per-sample Lp loss between the predicted x0 and a target, and its gradient (utils_Img2Img.py:699-751)
__device__ __forceinline__ float lp_x0(const pd_lp_guidance_args& a, float x, float o, bool& inside) {
  float x0 = a.pred_type == PD_PRED_EPSILON ? (x - a.sqrt_b * o) / a.sqrt_a : (a.pred_type == PD_PRED_SAMPLE ? o : a.sqrt_a * x - a.sqrt_b * o);
  inside = true;
  if (a.clip) { inside = x0 >= -a.clip_range && x0 <= a.clip_range; x0 = fminf(fmaxf(x0, -a.clip_range), a.clip_range); }
  return x0;
}

// grid = B * splits blocks of 256 threads: partial[n * splits + sp] = sum |x0 - target|^p over the block's share of sample n
__device__ __forceinline__ void lp_reduce_body(const pd_lp_guidance_args& a) {
  __shared__ double red[256];
  const int n = blockIdx.x / a.splits, sp = blockIdx.x % a.splits;
  const int64_t per = (a.per_sample + a.splits - 1) / a.splits;
  const int64_t lo = sp * per, hi = lo + per < a.per_sample ? lo + per : a.per_sample;
  double s = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const int64_t k = (int64_t)n * a.per_sample + i;
    bool in;
    const float d = lp_x0(a, a.sample[k], a.model_out[k], in) - a.target[k];
    s += (double)(a.p == 2.0f ? d * d : powf(fabsf(d), a.p));
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) a.partial[blockIdx.x] = red[0];
}

// same grid.  SCALED: d_model_out carries *grad_scale (read here, on the device); losses and d_sample_direct do not
template <bool SCALED>
__device__ __forceinline__ void lp_grad_body(const pd_lp_guidance_args& a, const float* grad_scale) {
  const int n = blockIdx.x / a.splits, sp = blockIdx.x % a.splits;
  double tot = 0.0;
  for (int k = 0; k < a.splits; ++k) tot += a.partial[n * a.splits + k];
  const float L = (float)pow(tot, 1.0 / (double)a.p);
  if (sp == 0 && threadIdx.x == 0 && a.losses) a.losses[n] = L;
  const float invL = L > 0.f ? 1.0f / (a.p == 2.0f ? L : powf(L, a.p - 1.0f)) : 0.f;
  // d x0 / d model_out and d x0 / d sample by prediction type (DDIMScheduler.step, A.7)
  const float dxo = a.pred_type == PD_PRED_EPSILON ? -a.sqrt_b / a.sqrt_a : (a.pred_type == PD_PRED_SAMPLE ? 1.0f : -a.sqrt_b);
  const float dxs = a.pred_type == PD_PRED_EPSILON ? 1.0f / a.sqrt_a : (a.pred_type == PD_PRED_SAMPLE ? 0.0f : a.sqrt_a);
  const float gs = SCALED ? grad_scale[0] : 1.0f;
  const int64_t per = (a.per_sample + a.splits - 1) / a.splits;
  const int64_t lo = sp * per, hi = lo + per < a.per_sample ? lo + per : a.per_sample;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const int64_t k = (int64_t)n * a.per_sample + i;
    bool in;
    const float d = lp_x0(a, a.sample[k], a.model_out[k], in) - a.target[k];
    float g = a.p == 2.0f ? d : copysignf(powf(fabsf(d), a.p - 1.0f), d);
    g = in ? g * invL : 0.f;               // clamp passes gradient only inside [-r, r]
    const float go = g * dxo;
    a.d_model_out[k] = SCALED ? go * gs : go;
    a.d_sample_direct[k] = g * dxs;
  }
}

// what both entry points refuse (`who`: the entry point's name, for the message)
static inline int lp_guidance_validate(const pd_lp_guidance_args* a, const char* who) {
  PD_CHECK(a != nullptr && a->numel > 0 && a->per_sample > 0 && a->numel % a->per_sample == 0, PD_ERR_ARG, "%s: bad sizes", who);
  PD_CHECK(a->sample && a->model_out && a->target && a->partial && a->d_model_out && a->d_sample_direct && a->splits >= 1, PD_ERR_ARG, "%s: null pointer", who);
  PD_CHECK(a->p >= 1.0f && a->p < 1e6f, PD_ERR_UNSUPPORTED, "%s: p = %g (finite p >= 1 only)", who, (double)a->p);
  PD_CHECK(a->pred_type >= 0 && a->pred_type <= 2, PD_ERR_ARG, "%s: bad prediction type", who);
  return PD_OK;
}

}  // namespace pd
