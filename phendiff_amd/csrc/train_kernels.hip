// Training-step building blocks: bandwidth-bound fused passes over flat fp32 buffers.
// The UNet backward itself is NOT built yet; these are the pieces around it.
//   pd_diffusion_loss : loss + dL/d(model_output) for epsilon / sample (SNR-weighted) / v_prediction  (utils_training.py:415-433)
//   pd_sumsq          : deterministic sum of squares of a flat buffer (global grad norm, utils_training.py:438-440)
//   pd_adamw_ema      : grad clip scaling + torch AdamW update + diffusers EMAModel.step in ONE pass  (:452-454, :553-556)
#include "pd_common.h"
#include "pd_guided.h"

namespace pd {

constexpr int RED_BLOCKS = 1024;

__device__ __forceinline__ double block_sum(double v, double* sm) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sm[i];
  return t;   // valid in thread 0
}

__global__ __launch_bounds__(256) void loss_kernel(const pd_loss_args a) {
#pragma clang fp contract(off)
  __shared__ double sm[4];
  double acc = 0.0;
  const float inv_n = 1.0f / (float)a.numel;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.numel; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / a.per_sample;
    float target, w = 1.0f;
    if (a.pred_type == PD_PRED_EPSILON) target = a.noise[i];
    else if (a.pred_type == PD_PRED_SAMPLE) { target = a.clean[i]; w = a.weight[n]; }
    else target = a.sa[n] * a.noise[i] - a.sb[n] * a.clean[i];      // get_velocity
    const float d = a.model_out[i] - target;
    acc += (double)(w * (d * d));
    if (a.grad_out) a.grad_out[i] = (2.0f * w * d) * inv_n * a.grad_scale;
  }
  const double t = block_sum(acc, sm);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void loss_finalize_kernel(const double* partial, int nblocks, double scale, float* out) {
  __shared__ double sm[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) acc += partial[i];
  const double t = block_sum(acc, sm);
  if (threadIdx.x == 0) out[0] = (float)(t * scale);
}

__global__ __launch_bounds__(256) void sumsq_kernel(const float* x, int64_t n, double* partial) {
  __shared__ double sm[4];
  double acc = 0.0;
  if ((((size_t)x) & 15) == 0) {
    // round 6: 16-byte loads, two in flight per lane (the 4-byte form ran the 3.46-GB gradient of the SD-2.1 UNet at 2.3 TB/s: 1.5 ms per step);
    // fixed summation order (deterministic), squares and sums in fp64 as before
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + stride < n4; i += 2 * stride) {
      const f32x4 a = ((const f32x4*)x)[i], b = ((const f32x4*)x)[i + stride];
#pragma unroll
      for (int j = 0; j < 4; ++j) { const double va = a[j], vb = b[j]; acc += va * va; acc += vb * vb; }
    }
    if (i < n4) {
      const f32x4 a = ((const f32x4*)x)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) { const double va = a[j]; acc += va * va; }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const double v = x[(n4 << 2) + threadIdx.x]; acc += v * v; }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { const double v = x[i]; acc += v * v; }
  }
  const double t = block_sum(acc, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// norm = sqrt(sum partial); clip coefficient as torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6))
__global__ __launch_bounds__(256) void norm_finalize_kernel(const double* partial, int nblocks, float max_norm, float* norm_out, float* coef_out) {
  __shared__ double sm[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) acc += partial[i];
  const double t = block_sum(acc, sm);
  if (threadIdx.x == 0) {
    const float nrm = (float)sqrt(t);
    norm_out[0] = nrm;
    const float c = max_norm / (nrm + 1e-6f);
    coef_out[0] = c < 1.0f ? c : 1.0f;
  }
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(const pd_adamw_ema_args a) {
#pragma clang fp contract(off)
  const float coef = a.clip_coef ? a.clip_coef[0] : 1.0f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.numel; i += (int64_t)gridDim.x * 256) {
    float p = a.param[i];
    if (a.ema_only) {                                                // a parameter whose .grad is None: torch skips its update
      if (a.ema) { const float s = a.ema[i]; a.ema[i] = s - a.one_minus_decay * (s - p); }
      if (a.zero_grad) a.grad[i] = 0.0f;
      continue;
    }
    const float g = a.grad[i] * coef;
    p = p * (1.0f - a.lr * a.weight_decay);                          // param.mul_(1 - lr * wd)
    const float m = a.exp_avg[i] + (g - a.exp_avg[i]) * (1.0f - a.beta1);   // exp_avg.lerp_(grad, 1 - beta1)
    const float v = a.exp_avg_sq[i] * a.beta2 + (g * g) * (1.0f - a.beta2);
    const float denom = sqrtf(v) / a.bias_correction2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);                               // addcdiv_(exp_avg, denom, value=-step_size)
    a.param[i] = p; a.exp_avg[i] = m; a.exp_avg_sq[i] = v;
    if (a.ema) { const float s = a.ema[i]; a.ema[i] = s - a.one_minus_decay * (s - p); }   // EMAModel.step
    if (a.zero_grad) a.grad[i] = 0.0f;
  }
}


// ---- gradient-guided transfer (utils_Img2Img.py:699-751): per-sample Lp loss between the predicted x0 and a target, and its
// gradient w.r.t. the UNet output and (directly) the sample.  The bodies live in pd_guided.h (pd_lp_guidance_scaled runs them too)
__global__ __launch_bounds__(256) void lp_reduce_kernel(const pd_lp_guidance_args a) { lp_reduce_body(a); }

__global__ __launch_bounds__(256) void lp_grad_kernel(const pd_lp_guidance_args a) { lp_grad_body<false>(a, nullptr); }

__global__ __launch_bounds__(256) void guidance_apply_kernel(const pd_guidance_apply_args a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.numel; i += (int64_t)gridDim.x * 256)
    a.out[i] = guidance_push(a.x[i], a.scale, a.g_direct[i], a.g_unet[i]);
}

}  // namespace pd

using namespace pd;

extern "C" int pd_diffusion_loss(const pd_loss_args* a, void* stream) {
  PD_CHECK(a != nullptr && a->numel > 0 && a->per_sample > 0 && a->numel % a->per_sample == 0, PD_ERR_ARG, "pd_diffusion_loss: bad sizes");
  PD_CHECK(a->model_out && a->partial && a->loss_out, PD_ERR_ARG, "pd_diffusion_loss: null pointer");
  PD_CHECK(a->pred_type >= 0 && a->pred_type <= 2, PD_ERR_ARG, "pd_diffusion_loss: bad prediction type");
  if (a->pred_type == PD_PRED_EPSILON) PD_CHECK(a->noise, PD_ERR_ARG, "pd_diffusion_loss: epsilon needs noise");
  if (a->pred_type == PD_PRED_SAMPLE) PD_CHECK(a->clean && a->weight, PD_ERR_ARG, "pd_diffusion_loss: sample needs clean + SNR weights");
  if (a->pred_type == PD_PRED_V) PD_CHECK(a->clean && a->noise && a->sa && a->sb, PD_ERR_ARG, "pd_diffusion_loss: v_prediction needs clean, noise, sa, sb");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_kernel, dim3(RED_BLOCKS), dim3(256), 0, st, *a);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)a->partial, RED_BLOCKS, 1.0 / (double)a->numel, a->loss_out);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_grad_norm(const float* grad, int64_t numel, double* partial, float max_norm, float* norm_out, float* clip_coef_out, void* stream) {
  PD_CHECK(grad && numel > 0 && partial && norm_out && clip_coef_out, PD_ERR_ARG, "pd_grad_norm: bad args");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sumsq_kernel, dim3(RED_BLOCKS), dim3(256), 0, st, grad, numel, partial);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, RED_BLOCKS, max_norm, norm_out, clip_coef_out);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_adamw_ema(const pd_adamw_ema_args* a, void* stream) {
  PD_CHECK(a != nullptr && a->numel > 0 && a->param && a->grad && a->exp_avg && a->exp_avg_sq, PD_ERR_ARG, "pd_adamw_ema: bad args");
  PD_CHECK(a->bias_correction2_sqrt > 0.f, PD_ERR_ARG, "pd_adamw_ema: bias_correction2_sqrt must be > 0");
  const int64_t blocks = (a->numel + 255) / 256;
  hipLaunchKernelGGL(adamw_ema_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_lp_guidance(const pd_lp_guidance_args* a, void* stream) {
  using namespace pd;
  if (const int rc = lp_guidance_validate(a, "pd_lp_guidance")) return rc;
  const unsigned grid = (unsigned)((a->numel / a->per_sample) * a->splits);
  hipLaunchKernelGGL(lp_reduce_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  hipLaunchKernelGGL(lp_grad_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_guidance_apply(const pd_guidance_apply_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr && a->numel > 0 && a->x && a->g_direct && a->g_unet && a->out, PD_ERR_ARG, "pd_guidance_apply: bad args");
  const unsigned grid = (unsigned)((a->numel + 255) / 256 < 4096 ? (a->numel + 255) / 256 : 4096);
  hipLaunchKernelGGL(guidance_apply_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
