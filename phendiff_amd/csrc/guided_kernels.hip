// Gradient-guided transfer as a captured trajectory (utils_Img2Img.py:699-760): the two launches of a guided step that the fp16 overflow
// protocol kept on the host.
//   pd_lp_guidance_scaled : pd_lp_guidance whose d_model_out carries the gradient scale, read from a DEVICE scalar (the runner halves it
//                           between replays without touching the captured launch)
//   pd_guided_step        : un-scale + finiteness test + `images - guidance_loss_scale * grad` + DDIMScheduler.step in ONE elementwise
//                           launch (was: mul_, isfinite().all() read on the host, pd_guidance_apply, pd_ddim_step)
// Both reuse the per-element arithmetic of the launches they replace (pd_guided.h): the results are those launches', bit for bit.
#include "pd_common.h"
#include "pd_guided.h"

namespace pd {

__global__ __launch_bounds__(256) void lp_reduce_scaled_kernel(const pd_lp_guidance_args a) { lp_reduce_body(a); }

__global__ __launch_bounds__(256) void lp_grad_scaled_kernel(const pd_lp_guidance_args a, const float* grad_scale) { lp_grad_body<true>(a, grad_scale); }

// 256 threads x 4 elements per block and pass; at most GUIDED_MAX_BLOCKS blocks (4 per CU), which walk a larger tensor in a grid-stride loop
constexpr int GUIDED_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void guided_step_kernel(const pd_guided_step_args a) {
#pragma clang fp contract(off)
  // 1 / scale on the device: exact for the powers of two the runner keeps, like the `mul_(1.0 / gscale)` this replaces
  const float inv = a.grad_scale ? 1.0f / a.grad_scale[0] : 1.0f;
  const int64_t stride = (int64_t)gridDim.x * 1024;
  bool bad = false;
  for (int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < a.numel; i0 += stride) {
    const int cnt = (int)min((int64_t)4, a.numel - i0);
    float x[4], o[4], gd[4], gu[4], xp[4], ps[4];
    if (cnt == 4) {
      const f32x4 vx = *(const f32x4*)(a.sample + i0), vo = *(const f32x4*)(a.model_out + i0);
      const f32x4 vd = *(const f32x4*)(a.g_direct + i0), vu = *(const f32x4*)(a.g_unet + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { x[j] = vx[j]; o[j] = vo[j]; gd[j] = vd[j]; gu[j] = vu[j]; }
    } else {      // the last, partial vector: nothing past numel is read (the lanes beyond it compute on zeros and store nothing)
      for (int j = 0; j < 4; ++j) {
        const bool in = j < cnt;
        x[j] = in ? a.sample[i0 + j] : 0.f; o[j] = in ? a.model_out[i0 + j] : 0.f;
        gd[j] = in ? a.g_direct[i0 + j] : 0.f; gu[j] = in ? a.g_unet[i0 + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bad |= !__builtin_isfinite(gu[j]);
      const float u = gu[j] * inv;                              // plan.dsample.mul_(1 / scale)
      ps[j] = guidance_push(x[j], a.guidance_scale, gd[j], u);  // pd_guidance_apply
      float x0;
      xp[j] = ddim_step_elem(a, ps[j], o[j], x0);               // pd_ddim_step(sample = pushed)
    }
    if (cnt == 4) {
      *(f32x4*)(a.prev_sample + i0) = (f32x4){xp[0], xp[1], xp[2], xp[3]};
      if (a.pushed) *(f32x4*)(a.pushed + i0) = (f32x4){ps[0], ps[1], ps[2], ps[3]};
    } else {
      for (int j = 0; j < cnt; ++j) { a.prev_sample[i0 + j] = xp[j]; if (a.pushed) a.pushed[i0 + j] = ps[j]; }
    }
  }
  // every thread that met a non-finite gradient stores the same 1 (an ordinary per-lane store, no atomic); nobody else touches the flag
  if (bad && a.overflow) a.overflow[0] = 1;
}

}  // namespace pd

using namespace pd;

extern "C" int pd_lp_guidance_scaled(const pd_lp_guidance_args* a, const float* grad_scale, void* stream) {
  if (const int rc = lp_guidance_validate(a, "pd_lp_guidance_scaled")) return rc;
  PD_CHECK(grad_scale != nullptr, PD_ERR_ARG, "pd_lp_guidance_scaled: grad_scale is NULL (a device scalar; pd_lp_guidance is the unscaled form)");
  PD_CHECK((uintptr_t)grad_scale % 4 == 0, PD_ERR_ARG, "pd_lp_guidance_scaled: grad_scale must be 4-byte aligned");
  const unsigned grid = (unsigned)((a->numel / a->per_sample) * a->splits);
  hipLaunchKernelGGL(lp_reduce_scaled_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  hipLaunchKernelGGL(lp_grad_scaled_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a, grad_scale);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_guided_step(const pd_guided_step_args* a, void* stream) {
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_guided_step: null args");
  PD_CHECK(a->numel > 0, PD_ERR_ARG, "pd_guided_step: numel = %lld (must be > 0)", (long long)a->numel);
  PD_CHECK(a->per_sample > 0 && a->numel % a->per_sample == 0, PD_ERR_ARG, "pd_guided_step: numel %lld is not a multiple of per_sample %lld",
           (long long)a->numel, (long long)a->per_sample);
  PD_CHECK(a->pred_type >= 0 && a->pred_type <= 2, PD_ERR_ARG, "pd_guided_step: bad prediction type %d", a->pred_type);
  const void* const ptrs[] = {a->sample, a->g_direct, a->g_unet, a->model_out, a->prev_sample, a->pushed};
  const char* const names[] = {"sample", "g_direct", "g_unet", "model_out", "prev_sample", "pushed"};
  for (int i = 0; i < 6; ++i) {
    PD_CHECK(ptrs[i] != nullptr || i == 5, PD_ERR_ARG, "pd_guided_step: %s is NULL", names[i]);
    // every tensor goes through f32x4 loads / stores (NULL `pushed` passes: 0 % 16 == 0)
    PD_CHECK((uintptr_t)ptrs[i] % 16 == 0, PD_ERR_ARG, "pd_guided_step: %s must be 16-byte aligned", names[i]);
  }
  PD_CHECK((uintptr_t)a->grad_scale % 4 == 0 && (uintptr_t)a->overflow % 4 == 0, PD_ERR_ARG, "pd_guided_step: grad_scale / overflow must be 4-byte aligned");
  const int64_t blocks = (a->numel + 1023) / 1024;
  const unsigned grid = (unsigned)(blocks < GUIDED_MAX_BLOCKS ? blocks : GUIDED_MAX_BLOCKS);
  hipLaunchKernelGGL(guided_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
