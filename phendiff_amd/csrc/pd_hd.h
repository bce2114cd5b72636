// Tile geometry of the templated head-dimension attention kernels (forward: attn_hd.hip, backward: attn_hd_bwd.hip): D is padded to the MFMA
// step in LDS and registers only -- DK = D rounded up to 16 for a contraction over d (row fragments), DV = D rounded up to 32 where d is the
// row of the result (transposed 32-row tiles).
#pragma once
#include "pd_common.h"
#include "pd_stage.h"
#include "pd_d64.h"

namespace pd {

template <typename T, int D> struct HD {
  typedef Elem<T> E;
  typedef typename E::Frag Frag;
  static constexpr int ES = E::BYTES;
  static constexpr int DK = (D + 15) / 16 * 16, DV = (D + 31) / 32 * 32;
  static constexpr int KS = DK / 16, NT = DV / 32, PPR = D / 8;           // k-steps of QK^T, row tiles of O^T, 8-element pieces per row
  // row pitches as D64's: K rows read as ds_read_b128 rows (odd multiple of 16 B), V rows as transposed 4-row blocks (odd multiple of 64 B)
  static constexpr int KP = DK * ES + 16;
  static constexpr int VP = ES == 2 ? (((DV * 2 + 63) / 64) | 1) * 64 : DV * 4 + 16;
  // keys per tile: 64; 32 at D = 160 (64 would take 83 968 B of LDS: one workgroup per CU, where the registers allow two) and in the
  // fp32 parity engine.  The file is built with the MFMA accumulators in VGPRs (build.sh): O, S and the softmax share one register class.
  static constexpr int KT = (ES == 2 && D <= 80) ? 64 : 32;
  static constexpr int KBYTES = KT * KP, VBYTES = KT * VP, LDS = 2 * (KBYTES + VBYTES);
  static constexpr int NP = KT * PPR, PIECES = (NP + 255) / 256;           // staging pieces per tensor and tile / per thread
  static __device__ __forceinline__ int vt_lane_off(int lane) {            // (D64::vt_lane_off with this pitch)
    if constexpr (ES == 2) {
      const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
      return (4 * (g >> 1) + q) * VP + (16 * (g & 1) + 4 * pp) * 2;
    } else {
      return (4 * (lane >> 5)) * VP + (lane & 31) * 4;
    }
  }
  static __device__ __forceinline__ Frag load_vt(const unsigned char* base) {
    if constexpr (ES == 2) {
      return D64<T>::load_vt2(base, base + 8 * VP);
    } else {
      Frag f;
#pragma unroll
      for (int j = 0; j < 4; ++j) { f.lo[j] = *(const float*)(base + j * VP); f.hi[j] = *(const float*)(base + (8 + j) * VP); }
      return f;
    }
  }
};

}  // namespace pd
