// The project's counter-based normal stream (defined in include/phendiff_hip.h, pd_train_sample): Philox4x32-10 and the Box-Muller
// transform of its words.  One definition for every kernel that draws from the stream (sample_kernels.hip, stream_noise.hip): the same
// inline functions, so the same bits.
#pragma once
#include "pd_common.h"

namespace pd {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct Words { uint32_t w[4]; };

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += PHILOX_W0; k1 += PHILOX_W1;      // (the key is bumped between rounds; the bump after the tenth is unused)
  }
  return Words{{c0, c1, c2, c3}};
}

// One Box-Muller pair from two words.  u = (2 k + 1) 2^-25 with k = x >> 8 has 25 significant bits: where 2 k + 1 >= 2^24 it is not an
// fp32 number, but 1 - u = (2^25 - (2 k + 1)) 2^-25 is, so ln u = log1p(-(1 - u)) there; the angle 2 u is likewise taken as 2 u - 2
// (cospi / sinpi have period 2).  Every argument below is exact; the error is that of logf / log1pf, sqrtf, sincospif and one product.
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& z_even, float& z_odd) {
  const uint32_t wa = 2u * (xa >> 8) + 1u, wb = 2u * (xb >> 8) + 1u;      // odd, < 2^25
  const float ln_u = wa < (1u << 24) ? logf((float)wa * 0x1p-25f) : log1pf(-(float)((1u << 25) - wa) * 0x1p-25f);
  const float r = sqrtf(-2.0f * ln_u);
  const float angle = wb < (1u << 24) ? (float)wb * 0x1p-24f : -(float)((1u << 25) - wb) * 0x1p-24f;      // in (-1, 1)
  float s, c;
  sincospif(angle, &s, &c);
  z_even = r * c;
  z_odd = r * s;
}

}  // namespace pd
