// 16-bit image stacks (plate-reader / sCMOS TIFFs: mode I;16 bands, often only 10 to 12 bits occupied).
//   pd_image_preprocess_bands16   pd_image_preprocess_bands (data_kernels.hip) for uint16 sources: Pillow's 16bpc bilinear resample bit for
//                                 bit, then an intensity window [lo, hi] -> [0, 1], Normalize and flips.
//   pd_band_histogram16           exact per-band value counts (what the window's percentiles are read from).
//   pd_postproc_bands16           the way back: float32 NCHW -> uint16 NHWC in the source's range.
// The resample is pd_resample.h's tiled resampler, the one under the 8-bit entries, at uint16 samples and float64 coefficients (ip_u16);
// its checks, plan, band-group choice and band kernel are shared too, and this file adds the window's null check and the entry point.
//
// Resample arithmetic (ImagingResampleHorizontal_16bpc / Vertical_16bpc): per output sample ONE double accumulator, ss = 0.0, then
// ss = ss + (double)src[first + k] * coef[k] for k in order, the product and the sum rounded separately (no FMA: see ip_u16), and the
// kernel's ISA holds no v_fma_f64.  out = clamp((int)(ss + 0.5), 0, 65535).  Horizontal pass first INTO uint16, then the vertical pass;
// an axis whose size does not change is skipped.
//
// The shared LDS plan (ip_make_plan) at 8-byte table entries and 2-byte samples:
//   tables     (32 * ksize_x + 8 * ksize_y) * 8 B   20.3 KiB at the 32 x limit on both axes (65 taps), 3.4 KiB at 1080 -> 256 (11 taps)
//   bounds     (32 + 8) * 2 * 4 B
//   inter      span_y rows x 32 * ci samples x 2 B   span_y <= 291 rows: 18.2 KiB for ONE band at the limit, 12.5 KiB for five at 1080 -> 256
//   out tile   8 x 32 * ci x 2 B
//   stage      R rows x (span_x * pixel_stride + 4) B
// At the limit on both axes one band takes 39.3 KiB before staging, so R rows of 2.1 KiB come out of the 64 KiB ceiling (R = 11, 62.1 KiB
// in all); five bands at 1080 -> 256 take 18.8 KiB before staging and R = 15 rows of 1.4 KiB: 39.6 KiB.
#include "pd_resample.h"

namespace pd {

// ---- pd_band_histogram16 -------------------------------------------------------------------------------------------------------------
// A band's whole histogram is 65536 x 4 B = 256 KiB: more than a CU's LDS.  With 16-BIT counters it is 128 KiB and fits, and a 16-bit
// counter cannot overflow when the workgroup counts at most 65535 samples.  So: one workgroup (1024 threads, 128 KiB of LDS, one per CU)
// counts ONE band of a chunk of 64512 pixels (63 rounds of 1024) with LDS atomics -- dword d holds bin d in its low half and bin
// d + 32768 in its high half, so a flush lane adds to two CONTIGUOUS runs of `counts` -- then adds its non-zero bins to the global
// histogram (integer atomics: exact, order-independent).  The global atomics are at most min(chunk, 65536) per workgroup and shrink with
// the number of distinct values (12-bit data: 1 in 16 samples).
// Contention worst case, the all-equal image: 64 lanes adding to one LDS word serialise, so a wave whose valid lanes all hold one value
// (a run of background) adds its lane count once, from one lane.
constexpr int H16_THREADS = 1024, H16_UNROLL = 9, H16_CHUNK = 7 * H16_UNROLL * H16_THREADS, H16_LDS = 32768 * 4;
static_assert(H16_CHUNK <= 65535, "a 16-bit counter must hold a whole chunk");

__global__ __launch_bounds__(H16_THREADS) void band_histogram16_kernel(const pd_band_histogram16_args a, const unsigned total, const int flat) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint32_t* const h = (uint32_t*)smem;
  const int tid = threadIdx.x, lane = tid & 63, c = blockIdx.y;
  for (int i = tid; i < H16_LDS / 16; i += H16_THREADS) ((uint4*)h)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  const unsigned p0 = blockIdx.x * (unsigned)H16_CHUNK;                 // < total < 2^32
  const unsigned cnt = total - p0 < (unsigned)H16_CHUNK ? total - p0 : (unsigned)H16_CHUNK;
  const unsigned hw = (unsigned)a.H * (unsigned)a.W, w = (unsigned)a.W;
  const unsigned char* const base = (const unsigned char*)a.x + 2 * c;
  // H16_UNROLL loads in flight per lane before the first one is counted (one at a time, a wave waits a whole L2 round trip per sample).
  // Every load is unconditional, from an index clamped into the chunk (cnt >= 1); `valid` masks what lies past its end.
  for (unsigned off = 0; off < cnt; off += H16_THREADS * H16_UNROLL) {  // (uniform trip count: the ballots below see whole waves)
    unsigned v[H16_UNROLL];
#pragma unroll
    for (int u = 0; u < H16_UNROLL; ++u) {
      const unsigned i = off + (unsigned)u * H16_THREADS + tid;
      const unsigned p = p0 + (i < cnt ? i : cnt - 1);
      size_t byte;
      if (flat) {
        byte = (size_t)p * (size_t)a.pixel_stride;
      } else {
        const unsigned n = p / hw, rem = p - n * hw, y = rem / w, x = rem - y * w;
        byte = (size_t)n * (size_t)a.image_stride + (size_t)y * (size_t)a.row_stride + (size_t)x * (size_t)a.pixel_stride;
      }
      v[u] = *(const unsigned short*)(base + byte);
    }
#pragma unroll
    for (int u = 0; u < H16_UNROLL; ++u) {
      const bool valid = off + (unsigned)u * H16_THREADS + tid < cnt;
      const unsigned long long act = __ballot(valid);
      if (act != 0ull) {
        const int leader = __ffsll((long long)act) - 1;
        const unsigned v0 = (unsigned)__shfl((int)v[u], leader);
        const unsigned long long same = __ballot(valid && v[u] == v0);
        if (same == act) {
          if (lane == leader) atomicAdd(&h[v0 & 32767u], (unsigned)__popcll(act) << ((v0 >> 15) << 4));
        } else if (valid) {
          atomicAdd(&h[v[u] & 32767u], 1u << ((v[u] >> 15) << 4));
        }
      }
    }
  }
  __syncthreads();
  unsigned int* const out = a.counts + (size_t)c * 65536;
  for (int d = tid; d < 32768; d += H16_THREADS) {
    const uint32_t word = h[d];
    const unsigned lo = word & 0xffffu, hi = word >> 16;
    if (lo) atomicAdd(out + d, lo);
    if (hi) atomicAdd(out + 32768 + d, hi);
  }
}

// ---- pd_postproc_bands16 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void postproc_bands16_kernel(const pd_postproc_bands16_args a, const long long total) {
#pragma clang fp contract(off)
  const long long hw = (long long)a.H * a.W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % a.C);
    const long long pix = i / a.C, n = pix / hw, r = pix - n * hw;
    const float x = a.x[(n * a.C + c) * hw + r];
    float f = x * a.std[c] + a.mean[c];                       // two roundings (contraction is off)
    f = !(f >= 0.0f) ? 0.0f : (f > 1.0f ? 1.0f : f);          // NaN -> 0
    const float lo = a.lo[c];
    const float v = rintf(f * (a.hi[c] - lo) + lo);
    a.y[i] = (unsigned short)(!(v >= 0.0f) ? 0 : (v > 65535.0f ? 65535 : (int)v));
  }
}

}  // namespace pd

using namespace pd;

extern "C" int pd_image_preprocess_bands16(const pd_image_preprocess_bands16_args* a, void* stream) {
  const char* const name = "pd_image_preprocess_bands16";
  PD_CHECK(a != nullptr && a->x && (a->y_f32 || a->y_u16), PD_ERR_ARG, "%s: null pointer (args, x, and at least one of y_f32 / y_u16)", name);
  PD_CHECK(!a->y_f32 || (a->lo && a->hi), PD_ERR_ARG, "%s: null lo / hi (fp32 [C], the intensity window) with y_f32", name);
  return ip_launch_bands<ip_u16>(a, name, 128, stream);
}

extern "C" int pd_band_histogram16(const pd_band_histogram16_args* a, void* stream) {
  const char* const name = "pd_band_histogram16";
  PD_CHECK(a != nullptr && a->x && a->counts, PD_ERR_ARG, "%s: null pointer (args, x, counts)", name);
  PD_CHECK(a->C >= 1 && a->C <= 32, PD_ERR_ARG, "%s: C must be in 1..32 (got %d)", name, a->C);
  PD_CHECK(((uintptr_t)a->x & 1) == 0, PD_ERR_ARG, "%s: x must be 2-byte aligned", name);
  PD_CHECK(a->N > 0 && a->H > 0 && a->W > 0, PD_ERR_SHAPE, "%s: N, H and W must be positive", name);
  const long long total = (long long)a->N * a->H * a->W;
  PD_CHECK((long long)a->H * a->W < (1ll << 32) && total < (1ll << 32), PD_ERR_SHAPE, "%s: N * H * W must be below 2^32 (got %lld)", name, total);
  PD_CHECK(a->pixel_stride >= 2 * a->C, PD_ERR_SHAPE, "%s: pixel_stride must be at least 2 * C bytes (got %d)", name, a->pixel_stride);
  PD_CHECK((a->pixel_stride & 1) == 0 && (a->row_stride & 1) == 0 && (a->N == 1 || (a->image_stride & 1) == 0), PD_ERR_SHAPE,
           "%s: pixel_stride, row_stride and image_stride are byte strides of uint16 samples and must be even", name);
  const long long row_bytes = (long long)a->W * a->pixel_stride;
  PD_CHECK(a->row_stride >= row_bytes, PD_ERR_SHAPE, "%s: row_stride smaller than W * pixel_stride", name);
  const long long image_bytes = (long long)(a->H - 1) * a->row_stride + row_bytes;
  PD_CHECK(a->N == 1 || a->image_stride >= image_bytes, PD_ERR_SHAPE, "%s: image_stride smaller than one image", name);
  // rows that follow each other without a gap (and images likewise) are one run of pixels: no division per sample
  const int flat = a->row_stride == row_bytes && (a->N == 1 || a->image_stride == image_bytes);
  static LdsAttr attr;
  PD_CHECK(ensure_lds(attr, band_histogram16_kernel, H16_LDS), PD_ERR_LAUNCH, "%s: cannot reserve %d bytes of LDS", name, H16_LDS);
  const dim3 grid((unsigned)((total + H16_CHUNK - 1) / H16_CHUNK), (unsigned)a->C);
  hipLaunchKernelGGL(band_histogram16_kernel, grid, dim3(H16_THREADS), H16_LDS, (hipStream_t)stream, *a, (unsigned)total, flat);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_postproc_bands16(const pd_postproc_bands16_args* a, void* stream) {
  const char* const name = "pd_postproc_bands16";
  PD_CHECK(a != nullptr && a->x && a->y && a->lo && a->hi && a->mean && a->std, PD_ERR_ARG, "%s: null pointer (args, x, y, lo, hi, mean, std)", name);
  PD_CHECK(a->C >= 1 && a->C <= 32, PD_ERR_ARG, "%s: C must be in 1..32 (got %d)", name, a->C);
  PD_CHECK(a->N > 0 && a->H > 0 && a->W > 0, PD_ERR_SHAPE, "%s: N, H and W must be positive", name);
  const long long total = (long long)a->N * a->C * a->H * a->W;
  PD_CHECK(total < (1ll << 40), PD_ERR_SHAPE, "%s: more than 2^40 elements", name);
  long long blocks = (total + 255) / 256;
  if (blocks > 1 << 20) blocks = 1 << 20;
  hipLaunchKernelGGL(postproc_bands16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a, total);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
