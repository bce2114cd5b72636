// Gradient-guided transfer as a captured trajectory (utils_Img2Img.py:699-760): the two launches of a guided step that the fp16 overflow
// protocol kept on the host.
//   pd_lp_guidance_scaled : pd_lp_guidance whose d_model_out carries the gradient scale, read from a DEVICE scalar (the runner halves it
//                           between replays without touching the captured launch)
//   pd_guided_step        : un-scale + finiteness test + `images - guidance_loss_scale * grad` + DDIMScheduler.step in ONE elementwise
//                           launch (was: mul_, isfinite().all() read on the host, pd_guidance_apply, pd_ddim_step)
// Both reuse the per-element arithmetic of the launches they replace (guidance_push and the lp_* bodies of pd_guided.h; ddim_step_elem of
// pd_step.h): the results are those launches', bit for bit.
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
    // Four input streams under ONE cnt == 4 branch, two outputs under another: this kernel keeps its own loop shape.  On load_quad /
    // store_quad (pd_step.h: a branch per stream, the same accesses) it measured 3.6 % slower per launch (docs/LAB_r27.md).
    const int cnt = quad_count(a.numel, i0);
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
  const char* const who = "pd_guided_step";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  if (const int rc = step_validate_common(a->numel, a->per_sample, a->pred_type, who, PD_ERR_ARG)) return rc;
  const NamedPtr tensors[] = {{"sample", a->sample}, {"g_direct", a->g_direct}, {"g_unet", a->g_unet}, {"model_out", a->model_out},
                              {"prev_sample", a->prev_sample}, {"pushed", a->pushed}};
  for (int i = 0; i < 5; ++i) PD_CHECK(tensors[i].p != nullptr, PD_ERR_ARG, "%s: %s is NULL", who, tensors[i].name);      // pushed: optional
  if (const int rc = step_check_aligned16(tensors, who)) return rc;
  PD_CHECK((uintptr_t)a->grad_scale % 4 == 0 && (uintptr_t)a->overflow % 4 == 0, PD_ERR_ARG, "%s: grad_scale / overflow must be 4-byte aligned", who);
  const int64_t blocks = (a->numel + 1023) / 1024;
  const unsigned grid = (unsigned)(blocks < GUIDED_MAX_BLOCKS ? blocks : GUIDED_MAX_BLOCKS);
  hipLaunchKernelGGL(guided_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
