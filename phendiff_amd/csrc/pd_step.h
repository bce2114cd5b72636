// What the scheduler-step kernels share, one definition each, so that launches which promise each other's bits cannot drift apart:
//   quad_count, load_quad, store_quad, quad_rows : four consecutive elements per thread of a dense fp32 tensor, and the row of each
//   guidance_combine, step_operands             : the classifier-free guidance combine; the operands of a step, formed once
//   ddim_x0_eps, ddim_prev, ddim_step_elem      : DDIM(Inverse)Scheduler.step for one element
//   threshold_limit                             : the dynamic clamp of DDIMScheduler(thresholding=True)
//   step_validate_common, step_check_aligned16  : what every step entry point refuses before it launches
//   Slot, load_slot, store_slot                 : a 16-byte slot addressed by the index WITHIN A SAMPLE
// Users: ddim_step_kernel, threshold_step_kernel<RAW>, multistep_step_kernel; guided_step_kernel (ddim_step_elem and quad_count, around
// a loop of its own); pd_guidance_rescale (guidance_combine, load_slot, store_slot); pd_contrast_mask (load_slot, store_slot; the quads in
// pd_class_contrast and pd_mask_blend); pd_sample_stats (load_slot).  The reductions those three share: pd_reduce.h.
//
// FP contraction is OFF in every function here, by a pragma of its own: the pragma is lexical and does not follow a function into its
// caller.  The reference evaluates these formulas as separate fp32 mul / sub / div torch ops, and epsilon-prediction divides by
// sqrt(alpha_bar) ~ 1e-5 near t = N, which amplifies a fused-vs-separate rounding difference of the numerator by 1e5.  With contraction
// off every op is the same IEEE operation the CPU performs.
#pragma once
#include "pd_common.h"

namespace pd {

// ---- four elements per thread: element i0 + j, j = 0..3, of a tensor of numel elements (i0 a multiple of 4, i0 < numel) ----------------
__device__ __forceinline__ int quad_count(int64_t numel, int64_t i0) { return (int)min((int64_t)4, numel - i0); }

// cnt == 4: one 16-byte access.  The last, partial vector: element accesses, nothing past numel is read or written (the lanes beyond it
// compute on zeros and store nothing).
__device__ __forceinline__ void load_quad(const float* p, int64_t i0, int cnt, float (&v)[4]) {
  if (cnt == 4) {
    const f32x4 q = *(const f32x4*)(p + i0);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q[j];
  } else {
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[i0 + j] : 0.f;
  }
}
__device__ __forceinline__ void store_quad(float* p, int64_t i0, int cnt, const float (&v)[4]) {
  if (cnt == 4) *(f32x4*)(p + i0) = (f32x4){v[0], v[1], v[2], v[3]};
  else for (int j = 0; j < cnt; ++j) p[i0 + j] = v[j];
}

// rows[j] = (i0 + j) / per_sample from ONE division, for every per_sample >= 1 (the row may change at any j, at every j when
// per_sample == 1).  Lanes past numel take element i0's row: row B would index one past w[B - 1] / quantile[B - 1].
__device__ __forceinline__ void quad_rows(int64_t i0, int64_t per_sample, int cnt, int64_t (&rows)[4]) {
  const int64_t b0 = i0 / per_sample;
  int64_t b = b0, rem = i0 - b0 * per_sample;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (rem == per_sample) { rem = 0; ++b; }
    ++rem;
    rows[j] = j < cnt ? b : b0;
  }
}

// ---- the operands of a step ----------------------------------------------------------------------------------------------------------------
// The classifier-free guidance combine of a conditional (o) and an unconditional (u) prediction, both equations: a subtraction, a
// multiplication and an addition each rounded on its own.  The step kernels reach it through step_operands and both passes of
// pd_guidance_rescale call it, so the cfg whose standard deviation is taken is bit for bit the cfg that is rescaled -- and the cfg a
// step kernel forms of the same operands.
__device__ __forceinline__ float guidance_combine(int guidance_cfg, float o, float u, float w) {
#pragma clang fp contract(off)
  return guidance_cfg ? (o + w * (o - u)) : (u + w * (o - u));
}

// x[j], out[j]: the sample and the (guidance-combined) model output of element i0 + j; row[j]: its sample.  `A`: any argument struct
// with numel, per_sample, sample, model_out, uncond_out, w, w_per_sample, guidance_cfg.  uncond_out is read only where it is given (the
// branch is uniform over the launch).
struct StepOperands { float x[4], out[4]; int64_t row[4]; int cnt; };

template <typename A>
__device__ __forceinline__ StepOperands step_operands(const A& a, const int64_t i0) {
#pragma clang fp contract(off)
  StepOperands r;
  r.cnt = quad_count(a.numel, i0);
  float u[4];
  // the two or three streams under ONE cnt == 4 branch (load_quad's two cases, written out): their 16-byte loads issue back to back
  if (r.cnt == 4) {
    const f32x4 vx = *(const f32x4*)(a.sample + i0), vo = *(const f32x4*)(a.model_out + i0);
#pragma unroll
    for (int j = 0; j < 4; ++j) { r.x[j] = vx[j]; r.out[j] = vo[j]; u[j] = 0.f; }
    if (a.uncond_out) { const f32x4 vu = *(const f32x4*)(a.uncond_out + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = vu[j]; }
  } else {
    for (int j = 0; j < 4; ++j) { r.x[j] = j < r.cnt ? a.sample[i0 + j] : 0.f; r.out[j] = j < r.cnt ? a.model_out[i0 + j] : 0.f;
      u[j] = (a.uncond_out && j < r.cnt) ? a.uncond_out[i0 + j] : 0.f; }
  }
  quad_rows(i0, a.per_sample, r.cnt, r.row);
  if (a.uncond_out) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float w = a.w_per_sample ? a.w[r.row[j]] : a.w[0];
      r.out[j] = guidance_combine(a.guidance_cfg, r.out[j], u[j], w);
    }
  }
  return r;
}

// ---- the update, per element -----------------------------------------------------------------------------------------------------------------
// In its two halves, around whatever limits x0 (the static clamp of ddim_step_elem, threshold_limit): the unclamped x0 with the predicted
// noise, and prev_sample from a limited x0.  `A`: any argument struct with pred_type, sqrt_a, sqrt_b (ddim_prev: + use_clipped_model_output,
// sqrt_ap, dir_coef; ddim_step_elem: + clip, clip_range).  ddim_step_elem returns prev_sample; `x0` = pred_original_sample.
template <typename A>
__device__ __forceinline__ void ddim_x0_eps(const A& a, float x, float out, float& x0, float& eps) {
#pragma clang fp contract(off)
  if (a.pred_type == PD_PRED_EPSILON) { x0 = (x - a.sqrt_b * out) / a.sqrt_a; eps = out; }
  else if (a.pred_type == PD_PRED_SAMPLE) { x0 = out; eps = (x - a.sqrt_a * x0) / a.sqrt_b; }
  else { x0 = a.sqrt_a * x - a.sqrt_b * out; eps = a.sqrt_a * out + a.sqrt_b * x; }
}
template <typename A>
__device__ __forceinline__ float ddim_prev(const A& a, float x, float x0, float eps) {
#pragma clang fp contract(off)
  if (a.use_clipped_model_output) eps = (x - a.sqrt_a * x0) / a.sqrt_b;
  return a.sqrt_ap * x0 + a.dir_coef * eps;
}
template <typename A>
__device__ __forceinline__ float ddim_step_elem(const A& a, float x, float out, float& x0) {
#pragma clang fp contract(off)
  float eps;
  ddim_x0_eps(a, x, out, x0, eps);
  if (a.clip) x0 = fminf(fmaxf(x0, -a.clip_range), a.clip_range);
  return ddim_prev(a, x, x0, eps);
}

// Dynamic thresholding: s = clamp(q, 1, sample_max_value) as torch.clamp(min = 1, max = sample_max_value) does it (min first; a NaN
// stays), then clamp(x0, -s, s) / s.  q: the row's quantile of |x0| (pd_abs_quantile).
__device__ __forceinline__ float threshold_limit(float x0, float q, float sample_max_value) {
#pragma clang fp contract(off)
  float s = q < 1.0f ? 1.0f : q;
  s = s > sample_max_value ? sample_max_value : s;
  return fminf(fmaxf(x0, -s), s) / s;
}

// ---- what the step entry points refuse (`who`: the entry point's name, for the message) -------------------------------------------------
// sizes answer `shape_code` (the entry point's own: PD_ERR_ARG or PD_ERR_SHAPE), the prediction type PD_ERR_ARG
static inline int step_validate_common(int64_t numel, int64_t per_sample, int pred_type, const char* who, int shape_code) {
  PD_CHECK(numel > 0, shape_code, "%s: numel = %lld (must be > 0)", who, (long long)numel);
  PD_CHECK(per_sample > 0 && numel % per_sample == 0, shape_code, "%s: numel %lld is not a multiple of per_sample %lld", who,
           (long long)numel, (long long)per_sample);
  PD_CHECK(pred_type >= 0 && pred_type <= 2, PD_ERR_ARG, "%s: bad prediction type %d", who, pred_type);
  return PD_OK;
}

// every tensor of a step goes through f32x4 loads / stores (a NULL optional one passes: 0 % 16 == 0)
struct NamedPtr { const char* name; const void* p; };
template <int N> static inline int step_check_aligned16(const NamedPtr (&tensors)[N], const char* who) {
  for (const NamedPtr& t : tensors) PD_CHECK((uintptr_t)t.p % 16 == 0, PD_ERR_ARG, "%s: %s must be 16-byte aligned", who, t.name);
  return PD_OK;
}

// ---- a slot = 16 bytes of elements, addressed by the index within a sample ------------------------------------------------------------------
// Which element a lane takes depends only on the element's index within its sample, never on the address: the 16-byte load is used where
// a slot of VEC elements lies whole inside the sample and is 16-byte aligned, element loads everywhere else, and both deliver the same
// values to the same lane (the lane level of pd_reduce.h's determinism rule).
template <typename T> struct Slot;
template <> struct Slot<float> {
  static constexpr int VEC = 4;
  static __device__ __forceinline__ void load16(const float* p, float (&v)[4]) {
    const f32x4 q = *(const f32x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = q[k];
  }
};
template <> struct Slot<bf16_t> {
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void load16(const bf16_t* p, float (&v)[8]) {
    const s16x8 q = *(const s16x8*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = bf2f((bf16_t)q[k]);
  }
};
template <> struct Slot<half_t> {
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void load16(const half_t* p, float (&v)[8]) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const h8 q = *(const h8*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (float)q[k];
  }
};

// the first min(cnt, VEC) elements at p (cnt <= 0: nothing is read); returns how many are valid
template <typename T> __device__ __forceinline__ int load_slot(const T* p, int cnt, float (&v)[Slot<T>::VEC]) {
  constexpr int VEC = Slot<T>::VEC;
  if (cnt >= VEC && ((uintptr_t)p & 15) == 0) {
    Slot<T>::load16(p, v);
    return VEC;
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) v[k] = k < cnt ? Elem<T>::to_f(p[k]) : 0.f;
  return cnt < 0 ? 0 : (cnt < VEC ? cnt : VEC);
}

// its counterpart for an fp32 output: the 16-byte store where the slot's four elements are all valid and p is 16-byte aligned, element
// stores of the first cnt elsewhere
__device__ __forceinline__ void store_slot(float* p, int cnt, const float (&v)[4]) {
  if (cnt == 4 && ((uintptr_t)p & 15) == 0) {
    *(f32x4*)p = (f32x4){v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (k < cnt) p[k] = v[k]; }
  }
}

}  // namespace pd
