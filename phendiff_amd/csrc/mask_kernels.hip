// Class-contrast masks and the masked blend (the DiffEdit recipe, arXiv 2210.11427, on the pixel tier).  Contract: include/phendiff_hip.h.
// Host side: phendiff_amd.masked (class_contrast_mask, mask_blend, masked_ddib, MaskedDDIBGraph).  Dense fp32 NCHW tensors, per_pixel = H * W.
//     pd_class_contrast   acc[s][p] = (first ? 0 : acc[s][p]) + (sum_c |a[s][c][p] - b[s][c][p]|) / C          one launch per noise draw
//     pd_contrast_mask    mean_s (fp64 sum, rounded once), limit = ratio * mean, map = fminf(acc, limit) / limit, mask = map > 0.5
//     pd_mask_blend       out[s][c][p] = mask[s][p] ? x[s][c][p] : keep[s][c][p]                                   a selection
//
// The house rules of pd_step.h and pd_reduce.h: fixed-order reductions and no atomics; a sample's result is a
// function of that sample alone; contraction off wherever a formula is restated on the CPU (tests/contrast_mask_ref.py); everything is
// validated before the launch; quads (quad_count, load_quad, store_quad, quad_rows) over the flat tensors of the two elementwise
// kernels, slots (load_slot: the index WITHIN A SAMPLE decides what a lane takes, never the address) in the reduction.
//
// pd_contrast_mask is pd_guidance_rescale's two launches on one tiling: a sample is cut into chunks of PD_CONTRAST_MASK_CHUNK pixels, a
// workgroup of 256 threads takes one (sample, chunk) at a time.
//   partial: the chunk's sum of acc in fp64 -> workspace [B][chunks]
//   apply:   every workgroup folds ITS sample's partials (all of them, in one order), makes mean and limit, and writes map / mask of its
//            chunk; the workgroup of a sample's chunk 0 walks the whole sample once more to count its mask (integers) for stats.
// Reduction order: pd_reduce.h's.  Traffic per pixel: acc read twice (three times with stats: the count reads 4 bytes per pixel from
// L2 -- 256 KiB per 256 x 256 sample), map and mask written once.
#include "pd_reduce.h"
#include "pd_step.h"

namespace pd {
namespace {

constexpr int CHUNK = PD_CONTRAST_MASK_CHUNK, ITERS = CHUNK / (256 * 4);
constexpr int64_t MAX_BLOCKS = 65536;      // more quads / (sample, chunk) pairs than this many blocks take are walked in a grid-stride loop
static_assert(CHUNK % (256 * 4) == 0, "a chunk is a whole number of passes of 256 threads x 4 elements");

// ---- pd_class_contrast ---------------------------------------------------------------------------------------------------------------------
// One thread per four consecutive elements of acc [B][per_pixel].  A quad that lies inside one sample reads a slot per channel plane and
// operand (16 bytes where the plane's four pixels are aligned, elements elsewhere); a quad a sample boundary cuts reads its elements one
// by one.  Both hand the same values to the same sums: the channel sum is in ascending c for every element.
__global__ __launch_bounds__(256) void class_contrast_kernel(const pd_class_contrast_args a) {
#pragma clang fp contract(off)
  const int64_t numel = a.B * a.per_pixel, pp = a.per_pixel, stride = (int64_t)gridDim.x * 1024;
  for (int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < numel; i0 += stride) {
    const int cnt = quad_count(numel, i0);
    int64_t rows[4];
    quad_rows(i0, pp, cnt, rows);
    bool one_sample = true;
#pragma unroll
    for (int j = 1; j < 4; ++j) one_sample = one_sample && rows[j] == rows[0];      // (lanes past numel carry rows[0])
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    if (one_sample) {
      const int64_t base = rows[0] * a.C * pp + (i0 - rows[0] * pp);
      for (int c = 0; c < a.C; ++c) {
        float va[4], vb[4];
        load_slot(a.a + base + c * pp, cnt, va);
        load_slot(a.b + base + c * pp, cnt, vb);
#pragma unroll
        for (int j = 0; j < 4; ++j) sum[j] = sum[j] + fabsf(va[j] - vb[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
          const int64_t base = rows[j] * a.C * pp + (i0 + j - rows[j] * pp);
          for (int c = 0; c < a.C; ++c) sum[j] = sum[j] + fabsf(a.a[base + c * pp] - a.b[base + c * pp]);
        }
      }
    }
    float old[4] = {0.f, 0.f, 0.f, 0.f}, r[4];
    if (!a.first) load_quad(a.acc, i0, cnt, old);      // (uniform) first: acc is not touched before it is written
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float m = sum[j] / (float)a.C;
      r[j] = a.first ? m : old[j] + m;
    }
    store_quad(a.acc, i0, cnt, r);
  }
}

// ---- pd_contrast_mask --------------------------------------------------------------------------------------------------------------------
struct MaskLaunch {
  pd_contrast_mask_args a;
  int64_t chunks, items;     // chunks per sample; items = B * chunks
  double* part;              // [B][chunks]
};

// the one place where a pixel's map value is formed: the apply pass's chunk and the count of stats see the same bits
__device__ __forceinline__ float contrast_map(float v, float limit, bool usable) {
#pragma clang fp contract(off)
  return usable ? fminf(v, limit) / limit : 0.f;
}

__global__ __launch_bounds__(256) void contrast_mask_partial_kernel(const MaskLaunch p) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const int t = threadIdx.x;
  for (int64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
    const ChunkTile tl = chunk_tile(item, p.chunks, p.a.per_pixel, CHUNK);
    const float* in = p.a.acc + tl.b * p.a.per_pixel + tl.j0;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int e0 = (i * 256 + t) * 4;
      float v[4];
      const int cnt = load_slot(in + e0, tl.rem - e0, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) { if (k < cnt) acc += (double)v[k]; }
    }
    acc = block_reduce<Sum>(acc, red);
    if (t == 0) p.part[item] = acc;
    __syncthreads();      // (red is written again by the next pair of a grid-stride walk)
  }
}

__global__ __launch_bounds__(256) void contrast_mask_apply_kernel(const MaskLaunch p) {
#pragma clang fp contract(off)
  __shared__ double red[256][1];
  __shared__ float mean_s, limit_s;
  __shared__ long long count_s[4];
  const pd_contrast_mask_args& a = p.a;
  const int t = threadIdx.x;
  for (int64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
    const ChunkTile tl = chunk_tile(item, p.chunks, a.per_pixel, CHUNK);
    double sum[1];      // the sample's sum, in thread 0
    run_fold(Ops<Sum>(), p.part + tl.b * p.chunks, p.chunks, red, sum);
    if (t == 0) {
      const float mean = (float)(sum[0] / (double)a.per_pixel);
      mean_s = mean;
      limit_s = a.ratio * mean;
    }
    __syncthreads();
    const float mean = mean_s, limit = limit_s;
    const bool usable = limit > 0.f && limit <= 3.402823466e38f;      // a finite positive number (false for NaN)
    const float* in = a.acc + tl.b * a.per_pixel;
    float* map = a.map ? a.map + tl.b * a.per_pixel : nullptr;
    uint8_t* mask = a.mask + tl.b * a.per_pixel;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int64_t e0 = tl.j0 + (i * 256 + t) * 4;
      float v[4], m[4];
      const int cnt = load_slot(in + e0, tl.rem - (i * 256 + t) * 4, v);
      uint32_t bits = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        m[k] = contrast_map(v[k], limit, usable);
        bits |= (m[k] > 0.5f ? 1u : 0u) << (8 * k);
      }
      if (map) store_slot(map + e0, cnt, m);
      if (cnt == 4 && ((uintptr_t)(mask + e0) & 3) == 0) {
        *(uint32_t*)(mask + e0) = bits;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (k < cnt) mask[e0 + k] = (uint8_t)((bits >> (8 * k)) & 1u); }
      }
    }
    if (a.stats && tl.j0 == 0) {      // (uniform over the workgroup) the sample's first chunk: count the sample's mask, in integers
      long long count = 0;
      for (int64_t e0 = (int64_t)t * 4; e0 < a.per_pixel; e0 += 1024) {
        const int64_t left = a.per_pixel - e0;
        float v[4];
        const int cnt = load_slot(in + e0, left < 4 ? (int)left : 4, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (k < cnt && contrast_map(v[k], limit, usable) > 0.5f) ++count; }
      }
      const long long total = block_reduce<Sum>(count, count_s);
      if (t == 0) {
        float* st = a.stats + tl.b * 3;
        st[0] = mean;
        st[1] = limit;
        st[2] = (float)((double)total / (double)a.per_pixel);
      }
    }
    __syncthreads();      // (red, mean_s, limit_s and count_s are written again by the next pair of a grid-stride walk)
  }
}

// ---- pd_mask_blend -----------------------------------------------------------------------------------------------------------------------
// One thread per four consecutive elements of the flat [B * C][per_pixel] tensors.  quad_rows gives each element's plane (s * C + c) from
// one division; the sample of the quad's first plane takes one more, and the (at most three) plane changes inside a quad are walked.
__global__ __launch_bounds__(256) void mask_blend_kernel(const pd_mask_blend_args a) {
  const int64_t pp = a.per_pixel, numel = a.B * a.C * pp, stride = (int64_t)gridDim.x * 1024;
  for (int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < numel; i0 += stride) {
    const int cnt = quad_count(numel, i0);
    int64_t planes[4];
    quad_rows(i0, pp, cnt, planes);
    const int64_t s0 = planes[0] / a.C;
    const int c0 = (int)(planes[0] - s0 * a.C);
    bool take[4];
    const uint8_t* m0 = a.mask + s0 * pp + (i0 - planes[0] * pp);
    if (cnt == 4 && planes[3] == planes[0] && ((uintptr_t)m0 & 3) == 0) {      // the quad lies in one plane: its four mask bytes in one load
      const uint32_t m = *(const uint32_t*)m0;
#pragma unroll
      for (int j = 0; j < 4; ++j) take[j] = ((m >> (8 * j)) & 0xffu) != 0;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int64_t s = s0;
        int c = c0 + (int)(planes[j] - planes[0]);      // (0..3 planes further on)
#pragma unroll
        for (int u = 0; u < 3; ++u) { if (c >= a.C) { c -= a.C; ++s; } }      // (C = 1: every plane further on is a sample further on)
        take[j] = j < cnt && a.mask[s * pp + (i0 + j - planes[j] * pp)] != 0;      // (lanes past numel read nothing)
      }
    }
    float x[4], k[4], r[4];
    load_quad(a.x, i0, cnt, x);      // (out may alias x or keep: both quads are read before the store)
    load_quad(a.keep, i0, cnt, k);
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = take[j] ? x[j] : k[j];
    store_quad(a.out, i0, cnt, r);
  }
}

// B, C, per_pixel of the two elementwise entry points: the flat tensor must be countable in an int64 with room to spare
int validate_bcp(int64_t B, int C, int64_t per_pixel, const char* who) {
  PD_CHECK(B >= 1, PD_ERR_SHAPE, "%s: B = %lld (must be >= 1)", who, (long long)B);
  PD_CHECK(C >= 1 && C <= 32, PD_ERR_SHAPE, "%s: C = %d (1 to 32 channels)", who, C);
  PD_CHECK(per_pixel >= 1, PD_ERR_SHAPE, "%s: per_pixel = %lld (must be >= 1)", who, (long long)per_pixel);
  PD_CHECK(per_pixel < (1ll << 62) / C / B, PD_ERR_SHAPE, "%s: B * C * per_pixel = %lld * %d * %lld does not fit 62 bits", who, (long long)B, C,
           (long long)per_pixel);
  return PD_OK;
}

unsigned quad_grid(int64_t numel) {
  const int64_t blocks = (numel + 1023) / 1024;
  return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

}  // namespace
}  // namespace pd

using namespace pd;

extern "C" int pd_class_contrast(const pd_class_contrast_args* a, void* stream) {
  const char* const who = "pd_class_contrast";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->a != nullptr && a->b != nullptr, PD_ERR_ARG, "%s: a / b is NULL (the two noise predictions)", who);
  PD_CHECK(a->acc != nullptr, PD_ERR_ARG, "%s: acc is NULL", who);
  if (const int rc = validate_bcp(a->B, a->C, a->per_pixel, who)) return rc;
  if (const int rc = step_check_aligned16({{"a", a->a}, {"b", a->b}, {"acc", a->acc}}, who)) return rc;
  hipLaunchKernelGGL(class_contrast_kernel, dim3(quad_grid(a->B * a->per_pixel)), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" size_t pd_contrast_mask_workspace(int64_t B, int64_t per_pixel) {
  return (size_t)(chunks_of(B, per_pixel, CHUNK) * B) * sizeof(double);
}

extern "C" int pd_contrast_mask(const pd_contrast_mask_args* a, void* stream) {
  const char* const who = "pd_contrast_mask";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->acc != nullptr, PD_ERR_ARG, "%s: acc is NULL", who);
  PD_CHECK(a->mask != nullptr, PD_ERR_ARG, "%s: mask is NULL", who);
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "%s: null workspace (pd_contrast_mask_workspace gives its size)", who);
  PD_CHECK(a->ratio > 0.0f && a->ratio <= 3.402823466e38f, PD_ERR_ARG, "%s: ratio = %g (must be a finite positive number)", who, (double)a->ratio);
  if (const int rc = step_check_aligned16({{"acc", a->acc}, {"map", a->map}}, who)) return rc;
  PD_CHECK((uintptr_t)a->stats % 4 == 0, PD_ERR_ARG, "%s: stats must be 4-byte aligned", who);
  PD_CHECK((uintptr_t)a->workspace % 8 == 0, PD_ERR_ARG, "%s: workspace must be 8-byte aligned", who);
  PD_CHECK(a->B >= 1, PD_ERR_SHAPE, "%s: B = %lld (must be >= 1)", who, (long long)a->B);
  PD_CHECK(a->per_pixel >= 1, PD_ERR_SHAPE, "%s: per_pixel = %lld (must be >= 1)", who, (long long)a->per_pixel);
  MaskLaunch p;
  p.a = *a;
  p.chunks = chunks_of(a->B, a->per_pixel, CHUNK);
  PD_CHECK(p.chunks > 0, PD_ERR_SHAPE, "%s: more than 2^31 - 1 chunks of %d pixels: split the batch", who, CHUNK);
  p.items = a->B * p.chunks;
  p.part = (double*)a->workspace;
  const unsigned grid = (unsigned)(p.items < MAX_BLOCKS ? p.items : MAX_BLOCKS);
  hipLaunchKernelGGL(contrast_mask_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(contrast_mask_apply_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_mask_blend(const pd_mask_blend_args* a, void* stream) {
  const char* const who = "pd_mask_blend";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->x != nullptr && a->keep != nullptr, PD_ERR_ARG, "%s: x / keep is NULL", who);
  PD_CHECK(a->mask != nullptr, PD_ERR_ARG, "%s: mask is NULL", who);
  PD_CHECK(a->out != nullptr, PD_ERR_ARG, "%s: out is NULL", who);
  if (const int rc = validate_bcp(a->B, a->C, a->per_pixel, who)) return rc;
  if (const int rc = step_check_aligned16({{"x", a->x}, {"keep", a->keep}, {"out", a->out}}, who)) return rc;
  hipLaunchKernelGGL(mask_blend_kernel, dim3(quad_grid(a->B * a->C * a->per_pixel)), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
