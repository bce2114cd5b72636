// pd_multistep_step: one update of a linear multistep solver of the diffusion ODE (DPM-Solver++ 2M and its noise-prediction twin;
// host side phendiff_amd.schedulers.DPMSolverMultistepScheduler / DPMSolverMultistepInverseScheduler), one fused elementwise launch on
// dense fp32 NCHW tensors, of the family of pd_ddim_step (small_kernels.hip) and pd_guided_step (guided_kernels.hip):
//     o    = model_out, or the guidance combine of model_out / uncond_out / w exactly as ddim_step_kernel forms it
//     m0   = form 0: x0(o) limited by the static clamp or by the dynamic threshold;   form 1: eps(o)      (ddim_x0_eps, pd_guided.h)
//     prev = a x + b m0 [+ c (m0 - m1)],   m1 = hist_in        hist_out = m0 [, pred_x0 = m0]
// The host computes a, b, c in fp64 and rounds them once; with c == 0 this is the first-order (DDIM) update in the solver's variable.
//
// c == 0: hist_in is NOT read (the branch is uniform over the launch).  The first step of a trajectory has no history, and in a replayed
// graph the buffer holds the last prediction of the previous replay -- or NaN: 0 * NaN would poison every replay.
//
// Which x0 is thresholded: as pd_ddim_step_threshold, the kernel recomputes x0 from sample / model_out (/ uncond_out) through ddim_x0_eps
// under the same contraction setting (off) after the same guidance combine as pd_ddim_raw_x0, so pd_ddim_raw_x0 -> pd_abs_quantile ->
// pd_multistep_step (pd_ddim_step_threshold_args and pd_multistep_step_args carrying the same sample / model_out / uncond_out / w /
// sqrt_a / sqrt_b / pred_type) thresholds bit for bit the x0 whose quantile was taken.
//
// Traffic per element: sample, model_out, hist_in in; prev_sample, hist_out out (5 streams of 4 bytes; 4 on a first step, +1 with guidance,
// +1 with pred_x0) against pd_ddim_step's 3 (+1, +1).  256 threads x 4 elements per block and pass, at most MS_MAX_BLOCKS blocks, which
// walk a tensor of more than 1024 x 1024 elements in a grid-stride loop.
#include "pd_guided.h"

namespace pd {

constexpr int MS_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void multistep_step_kernel(const pd_multistep_step_args a) {
#pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * 1024;
  const bool second = a.c != 0.0f;                                      // (uniform) false: hist_in is not touched
  for (int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < a.numel; i0 += stride) {
    const int cnt = (int)min((int64_t)4, a.numel - i0);
    float x[4], o[4], u[4], m1[4], xp[4], m0[4];
    if (cnt == 4) {
      const f32x4 vx = *(const f32x4*)(a.sample + i0), vo = *(const f32x4*)(a.model_out + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { x[j] = vx[j]; o[j] = vo[j]; u[j] = 0.f; m1[j] = 0.f; }
      if (a.uncond_out) { const f32x4 vu = *(const f32x4*)(a.uncond_out + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = vu[j]; }
      if (second) { const f32x4 vh = *(const f32x4*)(a.hist_in + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) m1[j] = vh[j]; }
    } else {      // the last, partial vector: nothing past numel is read (the lanes beyond it compute on zeros and store nothing)
      for (int j = 0; j < 4; ++j) {
        const bool in = j < cnt;
        x[j] = in ? a.sample[i0 + j] : 0.f; o[j] = in ? a.model_out[i0 + j] : 0.f;
        u[j] = (a.uncond_out && in) ? a.uncond_out[i0 + j] : 0.f;
        m1[j] = (second && in) ? a.hist_in[i0 + j] : 0.f;
      }
    }
    // the row of element i0 + j (lanes past numel take element i0's: row B would index one past w[B - 1] / quantile[B - 1])
    const int64_t b0 = i0 / a.per_sample;
    int64_t b = b0, rem = i0 - b0 * a.per_sample;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (rem == a.per_sample) { rem = 0; ++b; }
      ++rem;
      const int64_t row = j < cnt ? b : b0;
      float out = o[j];
      if (a.uncond_out) {
        const float w = a.w_per_sample ? a.w[row] : a.w[0];
        out = guidance_combine(a.guidance_cfg, o[j], u[j], w);
      }
      float x0, eps;
      ddim_x0_eps(a, x[j], out, x0, eps);
      float m;
      if (a.form == 0) {
        if (a.quantile) {
          float s = a.quantile[row];
          s = s < 1.0f ? 1.0f : s;                                      // torch.clamp(min = 1, max = sample_max_value): min first; NaN stays
          s = s > a.sample_max_value ? a.sample_max_value : s;
          x0 = fminf(fmaxf(x0, -s), s) / s;
        } else if (a.clip) {
          x0 = fminf(fmaxf(x0, -a.clip_range), a.clip_range);
        }
        m = x0;
      } else {
        m = eps;
      }
      float p = a.a * x[j] + a.b * m;
      if (second) p = p + a.c * (m - m1[j]);
      xp[j] = p;
      m0[j] = m;
    }
    if (cnt == 4) {
      *(f32x4*)(a.prev_sample + i0) = (f32x4){xp[0], xp[1], xp[2], xp[3]};
      *(f32x4*)(a.hist_out + i0) = (f32x4){m0[0], m0[1], m0[2], m0[3]};
      if (a.pred_x0) *(f32x4*)(a.pred_x0 + i0) = (f32x4){m0[0], m0[1], m0[2], m0[3]};
    } else {
      for (int j = 0; j < cnt; ++j) { a.prev_sample[i0 + j] = xp[j]; a.hist_out[i0 + j] = m0[j]; if (a.pred_x0) a.pred_x0[i0 + j] = m0[j]; }
    }
  }
}

}  // namespace pd

using namespace pd;

extern "C" int pd_multistep_step(const pd_multistep_step_args* a, void* stream) {
  const char* const who = "pd_multistep_step";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->numel > 0, PD_ERR_SHAPE, "%s: numel = %lld (must be > 0)", who, (long long)a->numel);
  PD_CHECK(a->per_sample > 0 && a->numel % a->per_sample == 0, PD_ERR_SHAPE, "%s: numel %lld is not a multiple of per_sample %lld", who,
           (long long)a->numel, (long long)a->per_sample);
  PD_CHECK(a->pred_type >= 0 && a->pred_type <= 2, PD_ERR_ARG, "%s: bad prediction type %d", who, a->pred_type);
  PD_CHECK(a->form == 0 || a->form == 1, PD_ERR_ARG, "%s: bad form %d (0: data prediction, 1: noise prediction)", who, a->form);
  PD_CHECK(a->sample && a->model_out, PD_ERR_ARG, "%s: sample / model_out is NULL", who);
  PD_CHECK(a->prev_sample != nullptr, PD_ERR_ARG, "%s: prev_sample is NULL", who);
  PD_CHECK(a->hist_out != nullptr, PD_ERR_ARG, "%s: hist_out is NULL", who);
  PD_CHECK(a->hist_in != nullptr || !(a->c != 0.0f), PD_ERR_ARG, "%s: hist_in is NULL with c = %g (a second-order step reads the history)", who,
           (double)a->c);
  PD_CHECK((const float*)a->hist_out != a->hist_in, PD_ERR_ARG, "%s: hist_out must not alias hist_in", who);
  PD_CHECK(!a->uncond_out || a->w, PD_ERR_ARG, "%s: guidance without weights", who);
  PD_CHECK(a->form == 0 || (!a->clip && !a->quantile), PD_ERR_ARG, "%s: the noise-prediction form (form = 1) has no clamp (clip = %d, quantile %s)",
           who, a->clip, a->quantile ? "given" : "NULL");
  PD_CHECK(a->form == 0 || !a->pred_x0, PD_ERR_ARG, "%s: pred_x0 is the data-prediction form's output (form = 1 stores eps to hist_out only)", who);
  // every tensor goes through f32x4 loads / stores (a NULL optional one passes: 0 % 16 == 0)
  PD_CHECK(((uintptr_t)a->sample % 16 == 0) && ((uintptr_t)a->model_out % 16 == 0) && ((uintptr_t)a->uncond_out % 16 == 0) &&
           ((uintptr_t)a->hist_in % 16 == 0) && ((uintptr_t)a->prev_sample % 16 == 0) && ((uintptr_t)a->hist_out % 16 == 0) &&
           ((uintptr_t)a->pred_x0 % 16 == 0), PD_ERR_ARG, "%s: tensors must be 16-byte aligned", who);
  PD_CHECK((uintptr_t)a->w % 4 == 0, PD_ERR_ARG, "%s: w must be 4-byte aligned", who);
  PD_CHECK((uintptr_t)a->quantile % 4 == 0, PD_ERR_ARG, "%s: quantile must be 4-byte aligned", who);
  PD_CHECK(!a->quantile || a->sample_max_value > 0.0f, PD_ERR_ARG, "%s: sample_max_value = %g (must be positive)", who, (double)a->sample_max_value);
  const int64_t blocks = (a->numel + 1023) / 1024;
  const unsigned grid = (unsigned)(blocks < MS_MAX_BLOCKS ? blocks : MS_MAX_BLOCKS);
  hipLaunchKernelGGL(multistep_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
