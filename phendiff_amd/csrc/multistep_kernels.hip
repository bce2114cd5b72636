// pd_multistep_step: one update of a linear multistep solver of the diffusion ODE (DPM-Solver++ 2M and its noise-prediction twin;
// host side phendiff_amd.schedulers.DPMSolverMultistepScheduler / DPMSolverMultistepInverseScheduler), one fused elementwise launch on
// dense fp32 NCHW tensors, of the family of pd_ddim_step (small_kernels.hip) and pd_guided_step (guided_kernels.hip):
//     x, o = the sample, and model_out or its guidance combine with uncond_out / w      (step_operands, pd_step.h: every step kernel's)
//     m0   = form 0: x0(o) limited by the static clamp or by the dynamic threshold;   form 1: eps(o)      (ddim_x0_eps, threshold_limit)
//     prev = a x + b m0 [+ c (m0 - m1)],   m1 = hist_in        hist_out = m0 [, pred_x0 = m0]
// The host computes a, b, c in fp64 and rounds them once; with c == 0 this is the first-order (DDIM) update in the solver's variable.
//
// c == 0: hist_in is NOT read (the branch is uniform over the launch).  The first step of a trajectory has no history, and in a replayed
// graph the buffer holds the last prediction of the previous replay -- or NaN: 0 * NaN would poison every replay.
//
// Which x0 is thresholded: as pd_ddim_step_threshold, the kernel recomputes x0 from the same step_operands through the same ddim_x0_eps
// under the same contraction setting (off) as pd_ddim_raw_x0, and limits it by the same threshold_limit, so pd_ddim_raw_x0 -> pd_abs_quantile ->
// pd_multistep_step (pd_ddim_step_threshold_args and pd_multistep_step_args carrying the same sample / model_out / uncond_out / w /
// sqrt_a / sqrt_b / pred_type) thresholds bit for bit the x0 whose quantile was taken.
//
// Traffic per element: sample, model_out, hist_in in; prev_sample, hist_out out (5 streams of 4 bytes; 4 on a first step, +1 with guidance,
// +1 with pred_x0) against pd_ddim_step's 3 (+1, +1).  256 threads x 4 elements per block and pass, at most MS_MAX_BLOCKS blocks, which
// walk a tensor of more than 1024 x 1024 elements in a grid-stride loop.
#include "pd_step.h"

namespace pd {

constexpr int MS_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void multistep_step_kernel(const pd_multistep_step_args a) {
#pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * 1024;
  const bool second = a.c != 0.0f;                                      // (uniform) false: hist_in is not touched
  for (int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < a.numel; i0 += stride) {
    const StepOperands r = step_operands(a, i0);
    float m1[4] = {0.f, 0.f, 0.f, 0.f}, xp[4], m0[4];
    if (second) load_quad(a.hist_in, i0, r.cnt, m1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x0, eps;
      ddim_x0_eps(a, r.x[j], r.out[j], x0, eps);
      float m;
      if (a.form == 0) {
        if (a.quantile) x0 = threshold_limit(x0, a.quantile[r.row[j]], a.sample_max_value);
        else if (a.clip) x0 = fminf(fmaxf(x0, -a.clip_range), a.clip_range);
        m = x0;
      } else {
        m = eps;
      }
      float p = a.a * r.x[j] + a.b * m;
      if (second) p = p + a.c * (m - m1[j]);
      xp[j] = p;
      m0[j] = m;
    }
    store_quad(a.prev_sample, i0, r.cnt, xp);
    store_quad(a.hist_out, i0, r.cnt, m0);
    if (a.pred_x0) store_quad(a.pred_x0, i0, r.cnt, m0);
  }
}

}  // namespace pd

using namespace pd;

extern "C" int pd_multistep_step(const pd_multistep_step_args* a, void* stream) {
  const char* const who = "pd_multistep_step";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  if (const int rc = step_validate_common(a->numel, a->per_sample, a->pred_type, who, PD_ERR_SHAPE)) return rc;
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
  if (const int rc = step_check_aligned16({{"sample", a->sample}, {"model_out", a->model_out}, {"uncond_out", a->uncond_out},
                                           {"hist_in", a->hist_in}, {"prev_sample", a->prev_sample}, {"hist_out", a->hist_out},
                                           {"pred_x0", a->pred_x0}}, who)) return rc;
  PD_CHECK((uintptr_t)a->w % 4 == 0, PD_ERR_ARG, "%s: w must be 4-byte aligned", who);
  PD_CHECK((uintptr_t)a->quantile % 4 == 0, PD_ERR_ARG, "%s: quantile must be 4-byte aligned", who);
  PD_CHECK(!a->quantile || a->sample_max_value > 0.0f, PD_ERR_ARG, "%s: sample_max_value = %g (must be positive)", who, (double)a->sample_max_value);
  const int64_t blocks = (a->numel + 1023) / 1024;
  const unsigned grid = (unsigned)(blocks < MS_MAX_BLOCKS ? blocks : MS_MAX_BLOCKS);
  hipLaunchKernelGGL(multistep_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
