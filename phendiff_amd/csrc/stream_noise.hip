// pd_stream_noise / pd_stream_advance: out = a * x + b * z with z drawn from pd_train_sample's stream at a position kept in DEVICE memory,
// so a captured launch draws new numbers on every replay (the contract is in include/phendiff_hip.h).  fp32 [B][per_sample] in and out.
#include "pd_philox.h"

namespace pd {
namespace {

struct StreamLaunch {
  pd_stream_noise_args a;
  uint64_t row_quads, nquads;      // Philox counters one row touches, and all rows together
  int small;                       // nquads < 2^31: 32-bit index arithmetic
};

__global__ __launch_bounds__(256) void stream_noise_kernel(const StreamLaunch p) {
#pragma clang fp contract(off)      // out = a * x + b * z: two products and one sum, as add_noise_kernel rounds them
  const pd_stream_noise_args& a = p.a;
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= p.nquads) return;
  const uint64_t b = p.small ? (uint64_t)((uint32_t)j / (uint32_t)p.row_quads) : j / p.row_quads;
  const uint64_t jq = j - b * p.row_quads;
  // the stream position: 16 bytes, the same for every thread of every launch between two pd_stream_advance
  const uint64_t seed = a.state[0], step = a.state[1] + a.index_offset + b;
  const uint64_t q = (a.elem_base >> 2) + jq;
  const uint32_t c3 = (((uint32_t)(step >> 32) & 0xFFFFu) << 16) | ((uint32_t)a.rank << 4) | (uint32_t)a.purpose;
  const Words w = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)step, c3, (uint32_t)seed, (uint32_t)(seed >> 32));
  float z[4];
  box_muller(w.w[0], w.w[1], z[0], z[1]);
  box_muller(w.w[2], w.w[3], z[2], z[3]);
  const float ca = a.sa ? a.sa[b] : a.a, cb = a.sa ? a.sb[b] : a.b;
  const int64_t per = a.per_sample;
  const int64_t e0 = (int64_t)(4 * jq) - (int64_t)(a.elem_base & 3);      // the quad's first element within row b
  const int64_t row = (int64_t)b * per;
  float* out = a.out + row;
  const float* x = a.x ? a.x + row : nullptr;
  if (e0 >= 0 && e0 + 4 <= per) {
    uintptr_t al = (uintptr_t)(out + e0);
    if (x) al |= (uintptr_t)(x + e0);
    if ((al & 15) == 0) {
      f32x4 o;
      if (x) {
        const f32x4 v = *(const f32x4*)(x + e0);
        o = (f32x4){ca * v[0] + cb * z[0], ca * v[1] + cb * z[1], ca * v[2] + cb * z[2], ca * v[3] + cb * z[3]};
      } else {
        o = (f32x4){cb * z[0], cb * z[1], cb * z[2], cb * z[3]};
      }
      *(f32x4*)(out + e0) = o;
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t e = e0 + k;
    if (e < 0 || e >= per) continue;
    out[e] = x ? ca * x[e] + cb * z[k] : cb * z[k];
  }
}

__global__ void stream_advance_kernel(uint64_t* state, uint64_t n) { state[1] += n; }

}  // namespace
}  // namespace pd

extern "C" int pd_stream_noise(const pd_stream_noise_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_stream_noise: null args");
  PD_CHECK(a->state != nullptr, PD_ERR_ARG, "pd_stream_noise: null state");
  PD_CHECK(a->out != nullptr, PD_ERR_ARG, "pd_stream_noise: null out");
  PD_CHECK(((uintptr_t)a->state & 7) == 0 && (((uintptr_t)a->out | (uintptr_t)a->x | (uintptr_t)a->sa | (uintptr_t)a->sb) & 3) == 0, PD_ERR_ARG,
           "pd_stream_noise: misaligned pointer (state: 8 bytes; x, out, sa, sb: 4 bytes)");
  PD_CHECK(a->rank >= 0 && a->rank < 4096, PD_ERR_ARG, "pd_stream_noise: rank %d outside [0, 4096)", a->rank);
  PD_CHECK(a->purpose >= 0 && a->purpose < 16 && a->purpose != 1, PD_ERR_ARG,
           "pd_stream_noise: purpose %d (0 .. 15 without 1, the timestep stream)", a->purpose);
  PD_CHECK((a->sa == nullptr) == (a->sb == nullptr), PD_ERR_ARG, "pd_stream_noise: coefficient tables need both sa and sb");
  PD_CHECK(a->B >= 1, PD_ERR_SHAPE, "pd_stream_noise: B = %lld (must be positive)", (long long)a->B);
  PD_CHECK(a->per_sample >= 1 && a->per_sample % 4 == 0, PD_ERR_SHAPE,
           "pd_stream_noise: per_sample = %lld (a positive multiple of 4)", (long long)a->per_sample);
  PD_CHECK(a->index_offset <= (1ull << 48) && (uint64_t)a->B <= (1ull << 48) - a->index_offset, PD_ERR_ARG,
           "pd_stream_noise: index_offset + B = %llu + %lld beyond 2^48, the counter's step field", (unsigned long long)a->index_offset,
           (long long)a->B);
  StreamLaunch p;
  p.a = *a;
  p.row_quads = ((a->elem_base & 3) + (uint64_t)a->per_sample + 3) / 4;
  PD_CHECK(a->per_sample < (1ll << 62) / a->B && p.row_quads < (1ull << 40) / (uint64_t)a->B, PD_ERR_SHAPE,
           "pd_stream_noise: grid too large (B = %lld rows of %llu counters): split the batch through index_offset or the rows through "
           "elem_base", (long long)a->B, (unsigned long long)p.row_quads);
  p.nquads = p.row_quads * (uint64_t)a->B;
  const uint64_t blocks = (p.nquads + 255) / 256;
  PD_CHECK(blocks < (1ull << 31), PD_ERR_SHAPE, "pd_stream_noise: grid too large (%llu blocks): split the batch through index_offset",
           (unsigned long long)blocks);
  p.small = p.nquads < (1ull << 31) ? 1 : 0;
  hipLaunchKernelGGL(stream_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_stream_advance(void* state, uint64_t n, void* stream) {
  using namespace pd;
  PD_CHECK(state != nullptr && ((uintptr_t)state & 7) == 0, PD_ERR_ARG, "pd_stream_advance: null or misaligned state");
  hipLaunchKernelGGL(stream_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (uint64_t*)state, n);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
