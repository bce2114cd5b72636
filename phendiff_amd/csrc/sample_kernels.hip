// pd_train_sample: the training step's noise, timesteps and noisy sample in one launch, from a counter-based generator
// (Philox4x32-10; the stream is defined in include/phendiff_hip.h).  fp32 NCHW in and out, like pd_add_noise.
#include "pd_philox.h"

namespace pd {
namespace {

struct Launch {
  pd_train_sample_args a;
  uint64_t total, nquads;
  uint32_t k0, k1, c2, c3;      // key, counter words 2 and 3 (purpose bits clear)
  int want_t;                   // timesteps are needed (clean or timesteps_out given)
  int small;                    // total < 2^31: 32-bit index arithmetic
};

__device__ __forceinline__ int64_t timestep_of(const Launch& p, int64_t b) {
  if (p.a.timesteps_in) return p.a.timesteps_in[b];
  const Words t = philox4x32_10((uint32_t)b, (uint32_t)((uint64_t)b >> 32), p.c2, p.c3 | 1u, p.k0, p.k1);
  return (int64_t)__umulhi(t.w[0], (uint32_t)p.a.N);
}

__global__ __launch_bounds__(256) void train_sample_kernel(const Launch p) {
#pragma clang fp contract(off)      // noisy = sa * clean + sb * noise exactly as add_noise_kernel rounds it
  const pd_train_sample_args& a = p.a;
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= p.nquads) return;
  const uint64_t q = (a.elem_base >> 2) + j;
  const Words x = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), p.c2, p.c3 | (uint32_t)a.purpose, p.k0, p.k1);
  float z[4];
  box_muller(x.w[0], x.w[1], z[0], z[1]);
  box_muller(x.w[2], x.w[3], z[2], z[3]);
  const int64_t total = (int64_t)p.total, per = a.per_sample;
  const int64_t i0 = (int64_t)(4 * j) - (int64_t)(a.elem_base & 3);      // index of the quad's first element in this launch's buffers
  const bool whole = i0 >= 0 && i0 + 4 <= total;
  if (whole) {
    const int64_t b = p.small ? (int64_t)((uint32_t)i0 / (uint32_t)per) : i0 / per;
    const int64_t off = i0 - b * per;
    uintptr_t al = (uintptr_t)(a.noise + i0);
    if (a.clean) al |= (uintptr_t)(a.clean + i0) | (uintptr_t)(a.noisy + i0);
    if (off + 4 <= per && (al & 15) == 0) {      // inside one sample, 16-byte aligned everywhere
      *(f32x4*)(a.noise + i0) = (f32x4){z[0], z[1], z[2], z[3]};
      if (!p.want_t) return;
      const int64_t t = timestep_of(p, b);
      if (off == 0 && a.timesteps_out && !a.timesteps_in) a.timesteps_out[b] = t;
      if (!a.clean) return;
      const int ti = (int)(t < 0 ? 0 : (t >= a.N ? a.N - 1 : t));
      const float sa = a.sqrt_acp[ti], sb = a.sqrt_1m_acp[ti];
      const f32x4 c = *(const f32x4*)(a.clean + i0);
      *(f32x4*)(a.noisy + i0) = (f32x4){sa * c[0] + sb * z[0], sa * c[1] + sb * z[1], sa * c[2] + sb * z[2], sa * c[3] + sb * z[3]};
      return;
    }
  }
  int64_t b_prev = -1, t = 0;
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = i0 + k;
    if (i < 0 || i >= total) continue;
    a.noise[i] = z[k];
    if (!p.want_t) continue;
    const int64_t b = p.small ? (int64_t)((uint32_t)i / (uint32_t)per) : i / per;
    if (b != b_prev) {
      b_prev = b;
      t = timestep_of(p, b);
      if (a.clean) {
        const int ti = (int)(t < 0 ? 0 : (t >= a.N ? a.N - 1 : t));
        sa = a.sqrt_acp[ti]; sb = a.sqrt_1m_acp[ti];
      }
    }
    if (i == b * per && a.timesteps_out && !a.timesteps_in) a.timesteps_out[b] = t;
    if (a.clean) a.noisy[i] = sa * a.clean[i] + sb * z[k];
  }
}

}  // namespace
}  // namespace pd

extern "C" int pd_train_sample(const pd_train_sample_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_train_sample: null args");
  PD_CHECK(a->noise != nullptr, PD_ERR_ARG, "pd_train_sample: null noise output");
  PD_CHECK(a->rank >= 0 && a->rank < 4096, PD_ERR_ARG, "pd_train_sample: rank %d outside [0, 4096)", a->rank);
  PD_CHECK(a->step < (1ull << 48), PD_ERR_ARG, "pd_train_sample: step %llu outside [0, 2^48)", (unsigned long long)a->step);
  PD_CHECK(a->purpose >= 0 && a->purpose < 16 && a->purpose != 1, PD_ERR_ARG,
           "pd_train_sample: purpose %d (0 noise, 2 posterior noise / randn, up to 15; 1 is the timestep stream)", a->purpose);
  PD_CHECK(a->B > 0 && a->per_sample > 0, PD_ERR_SHAPE, "pd_train_sample: B and per_sample must be positive");
  PD_CHECK(a->B < (1ll << 31) && a->per_sample < (1ll << 62) / a->B && a->elem_base < (1ull << 62), PD_ERR_SHAPE,
           "pd_train_sample: B * per_sample and elem_base must stay below 2^62");
  const bool want_t = a->clean != nullptr || a->timesteps_out != nullptr;
  if (a->clean) {
    PD_CHECK(a->sqrt_acp && a->sqrt_1m_acp, PD_ERR_ARG, "pd_train_sample: clean without the sqrt_acp / sqrt_1m_acp tables");
    PD_CHECK(a->noisy != nullptr, PD_ERR_ARG, "pd_train_sample: null noisy output (clean is given)");
    PD_CHECK(a->timesteps_in || a->timesteps_out, PD_ERR_ARG, "pd_train_sample: null timesteps output (clean is given, timesteps_in is not)");
  } else {
    PD_CHECK(a->noisy == nullptr, PD_ERR_ARG, "pd_train_sample: noisy without clean");
  }
  PD_CHECK(!want_t || a->N > 0, PD_ERR_ARG, "pd_train_sample: N = %d timesteps (must be positive)", a->N);
  Launch p;
  p.a = *a;
  p.total = (uint64_t)a->B * (uint64_t)a->per_sample;
  p.nquads = ((a->elem_base & 3) + p.total + 3) / 4;
  const uint64_t blocks = (p.nquads + 255) / 256;
  PD_CHECK(blocks < (1ull << 31), PD_ERR_SHAPE, "pd_train_sample: grid too large (%llu blocks): split the tensor through elem_base",
           (unsigned long long)blocks);
  p.k0 = (uint32_t)a->seed; p.k1 = (uint32_t)(a->seed >> 32);
  p.c2 = (uint32_t)a->step;
  p.c3 = ((uint32_t)(a->step >> 32) << 16) | ((uint32_t)a->rank << 4);
  p.want_t = want_t ? 1 : 0;
  p.small = p.total < (1ull << 31) ? 1 : 0;
  hipLaunchKernelGGL(train_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
