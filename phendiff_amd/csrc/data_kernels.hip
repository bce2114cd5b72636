// Image preprocessing: decoded uint8 images -> the engine's float32 NCHW input (and the uint8 "raw" twin of the metric reference sets).
//   pd_image_preprocess   Resize(BILINEAR) -> ToTensor -> Normalize [-> RandomHorizontalFlip -> RandomVerticalFlip] of
//                         src/utils_dataset.py:104-127 and src/utils_Img2Img.py:197-206, which the reference runs per image in PIL on the host.
//   pd_image_preprocess_bands   the same transform for stacks of 1..32 independent bands (C in, C out).
// The resize is Pillow's 8-bit bilinear resample restated in the same integer arithmetic (ImagingResample: separable, antialiasing support
// max(scale, 1), 22-bit fixed-point coefficients, accumulator 1 << 21, >> 22, clamp; horizontal pass first INTO uint8, then the vertical
// pass; an axis whose size does not change is skipped, not run through an identity table), so the output is held to bit equality.  The
// host builds the coefficient tables in float64 (phendiff_amd/data.py resample_tables) and passes them in.
// The tiled resampler, its LDS plan, the argument checks and the band kernel are pd_resample.h's, shared with the 16-bit entry
// (data16_kernels.hip); this file holds the RGB / grey kernel, whose output stage replicates one channel to three, and the two entry points.
// A tile is written as uint8 NHWC bytes and / or converted ((float)v / 255 - mean) / std and written NCHW at the mirrored position.
#include "pd_resample.h"

namespace pd {

template <int CI>
__global__ __launch_bounds__(IP_THREADS) void image_preprocess_kernel(const pd_image_preprocess_args a, const ip_plan P) {
#pragma clang fp contract(off)      // ToTensor / Normalize are separate fp32 div, sub, div torch ops: keep them separate IEEE operations
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int slot = a.out_index ? a.out_index[n] : n;
  if (slot < 0 || slot >= a.out_slots) return;       // (uniform over the workgroup)
  const int ox0 = blockIdx.x * IP_TOW, oy0 = blockIdx.y * IP_TOH;
  const int tw = min(IP_TOW, a.OW - ox0), th = min(IP_TOH, a.OH - oy0);
  const unsigned char* const outt = ip_resample_tile<ip_u8, CI>(a, P, smem, n, 0, CI, ox0, oy0, tw, th);

  // ---- outputs
  if (a.y_u8) {                      // uint8 NHWC: each tile row is tw * 3 contiguous bytes
    const int per_row = tw * 3;
    for (int idx = tid; idx < th * per_row; idx += IP_THREADS) {
      const int oy = idx / per_row, j = idx - oy * per_row;
      const unsigned char v = outt[oy * P.irow + (CI == 3 ? j : j / 3)];
      a.y_u8[(((size_t)slot * a.OH + (oy0 + oy)) * a.OW + ox0) * 3 + j] = v;
    }
  }
  if (a.y_f32) {                     // float32 NCHW: consecutive lanes write consecutive (or, mirrored, reversed) columns of one row
    const int flip = a.flips ? a.flips[n] : 0;
    const int per_ch = th * tw;
    for (int idx = tid; idx < 3 * per_ch; idx += IP_THREADS) {
      const int c = idx / per_ch, rem = idx - c * per_ch;
      const int oy = rem / tw, ox = rem - oy * tw;
      const unsigned char v = outt[oy * P.irow + (CI == 3 ? ox * 3 + c : ox)];
      const float mean = c == 0 ? a.mean0 : (c == 1 ? a.mean1 : a.mean2);
      const float sd = c == 0 ? a.std0 : (c == 1 ? a.std1 : a.std2);
      const float f = ((float)v / 255.0f - mean) / sd;
      const int dx = (flip & 1) ? a.OW - 1 - (ox0 + ox) : ox0 + ox;
      const int dy = (flip & 2) ? a.OH - 1 - (oy0 + oy) : oy0 + oy;
      a.y_f32[(((size_t)slot * 3 + c) * a.OH + dy) * a.OW + dx] = f;
    }
  }
}

}  // namespace pd

using namespace pd;

extern "C" int pd_image_preprocess(const pd_image_preprocess_args* a, void* stream) {
  PD_CHECK(a != nullptr && a->x && (a->y_f32 || a->y_u8), PD_ERR_ARG, "pd_image_preprocess: null pointer (x, and at least one of y_f32 / y_u8)");
  PD_CHECK(a->Cin == 1 || a->Cin == 3, PD_ERR_ARG, "pd_image_preprocess: Cin must be 1 or 3 (got %d)", a->Cin);
  const int rc = ip_check(a, "pd_image_preprocess", 1, a->Cin, 3, a->Cin, "Cin", 8);
  if (rc != PD_OK) return rc;
  const bool rx = a->W != a->OW, ry = a->H != a->OH;
  ip_plan P;
  PD_CHECK(ip_make_plan(a->H, a->W, a->OH, a->OW, a->pixel_stride, a->Cin, rx ? a->ksize_x : 0, ry ? a->ksize_y : 0, 1, sizeof(int), &P),
           PD_ERR_SHAPE, "pd_image_preprocess: tile does not fit the LDS budget");
  const dim3 grid((unsigned)((a->OW + IP_TOW - 1) / IP_TOW), (unsigned)((a->OH + IP_TOH - 1) / IP_TOH), (unsigned)a->N);
  hipStream_t st = (hipStream_t)stream;
  if (a->Cin == 3) hipLaunchKernelGGL(image_preprocess_kernel<3>, grid, dim3(IP_THREADS), P.lds_bytes, st, *a, P);
  else hipLaunchKernelGGL(image_preprocess_kernel<1>, grid, dim3(IP_THREADS), P.lds_bytes, st, *a, P);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_image_preprocess_bands(const pd_image_preprocess_bands_args* a, void* stream) {
  PD_CHECK(a != nullptr && a->x && (a->y_f32 || a->y_u8), PD_ERR_ARG,
           "pd_image_preprocess_bands: null pointer (x, and at least one of y_f32 / y_u8)");
  return ip_launch_bands<ip_u8>(a, "pd_image_preprocess_bands", 64, stream);
}
