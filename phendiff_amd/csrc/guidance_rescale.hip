// pd_guidance_rescale: classifier-free guidance with the guided prediction brought back towards the conditional prediction's per-sample
// standard deviation (arXiv 2305.08891 section 3.4; diffusers' rescale_noise_cfg), on dense fp32 [B][n] tensors.  Contract:
// include/phendiff_hip.h.  Host side: phendiff_amd.schedulers.GuidanceRescale.
//     cfg = guidance_combine(cond, uncond, w)   (pd_step.h: the step kernels' expression; load_slot is there too)
//     g_b = phi * std(cond_b) / std(cfg_b) + (1 - phi)   (fp64, rounded to fp32 once)          out = cfg * g_b
//
// Two launches on one stream, no host synchronisation, the same tiling in both: a sample is cut into chunks of
// PD_GUIDANCE_RESCALE_CHUNK elements and a workgroup of 256 threads takes one (sample, chunk) at a time.
//   partial: sum cond, sum cond^2, sum cfg, sum cfg^2 of the chunk in fp64 -> workspace [B][chunks][4]
//   apply:   every workgroup folds ITS sample's partials (all of them, in one order), makes g_b, and writes cfg * g_b for its chunk
// The fold is repeated by each of a sample's workgroups instead of being a launch of its own: it reads 32 bytes per chunk (768 bytes for a
// 3 x 256 x 256 image) from L2, against the 96 KiB the workgroup streams.  Traffic per element: cond and uncond read twice, out written once.
//
// Determinism: the reductions run in the one fixed order of pd_reduce.h, and which element a lane takes depends only on the element's
// index WITHIN ITS SAMPLE (load_slot / store_slot).  So a sample's g does not depend on B, on its row in the batch, on its alignment, on
// the grid or on the replay.
#include "pd_reduce.h"
#include "pd_step.h"

namespace pd {
namespace {

constexpr int CHUNK = PD_GUIDANCE_RESCALE_CHUNK, ITERS = CHUNK / (256 * 4), NSUM = 4;
using Sums = Ops<Sum, Sum, Sum, Sum>;      // sum cond, sum cond^2, sum cfg, sum cfg^2
constexpr int64_t MAX_BLOCKS = 65536;      // more (sample, chunk) pairs than this are walked in a grid-stride loop
static_assert(CHUNK % (256 * 4) == 0, "a chunk is a whole number of passes of 256 threads x 4 elements");

struct Launch {
  pd_guidance_rescale_args a;
  int64_t chunks, items;     // chunks per sample; items = B * chunks
  double* part;              // [B][chunks][NSUM]
};

__global__ __launch_bounds__(256) void guidance_rescale_partial_kernel(const Launch p) {
#pragma clang fp contract(off)
  __shared__ double red[4][NSUM];
  const pd_guidance_rescale_args& a = p.a;
  const int t = threadIdx.x;
  for (int64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
    const ChunkTile tl = chunk_tile(item, p.chunks, a.per_sample, CHUNK);
    const int64_t off = tl.b * a.per_sample + tl.j0;
    const float* co = a.model_out + off;
    const float* un = a.uncond_out + off;
    const float w = a.w_per_sample ? a.w[tl.b] : a.w[0];
    double acc[NSUM] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int e0 = (i * 256 + t) * 4;
      float o[4], u[4];
      const int cnt = load_slot(co + e0, tl.rem - e0, o);
      load_slot(un + e0, tl.rem - e0, u);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
          const double c = (double)o[k], g = (double)guidance_combine(a.guidance_cfg, o[k], u[k], w);
          acc[0] += c;
          acc[1] += c * c;      // (exact: 48 significant bits at most)
          acc[2] += g;
          acc[3] += g * g;
        }
      }
    }
    block_reduce(Sums(), acc, red);
    if (t == 0) {
#pragma unroll
      for (int i = 0; i < NSUM; ++i) p.part[item * NSUM + i] = acc[i];
    }
    __syncthreads();      // (red is written again by the next pair of a grid-stride walk)
  }
}

__global__ __launch_bounds__(256) void guidance_rescale_apply_kernel(const Launch p) {
#pragma clang fp contract(off)
  __shared__ double red[256][NSUM];
  __shared__ float g_s;
  const pd_guidance_rescale_args& a = p.a;
  const int t = threadIdx.x;
  for (int64_t item = blockIdx.x; item < p.items; item += gridDim.x) {
    const ChunkTile tl = chunk_tile(item, p.chunks, a.per_sample, CHUNK);
    const int64_t off = tl.b * a.per_sample + tl.j0;
    double s[NSUM];      // the sample's four sums, in thread 0
    run_fold(Sums(), p.part + tl.b * p.chunks * NSUM, p.chunks, red, s);
    if (t == 0) {
      const double n = (double)a.per_sample, phi = (double)a.rescale;
      double var_c = (s[1] - s[0] * s[0] / n) / (n - 1.0), var_g = (s[3] - s[2] * s[2] / n) / (n - 1.0);
      var_c = var_c < 0.0 ? 0.0 : var_c;      // (rounding below zero of a constant row; a NaN stays)
      var_g = var_g < 0.0 ? 0.0 : var_g;
      g_s = (float)(phi * (sqrt(var_c) / sqrt(var_g)) + (1.0 - phi));
    }
    __syncthreads();
    const float g = g_s;
    const float* co = a.model_out + off;
    const float* un = a.uncond_out + off;
    float* out = a.out + off;
    const float w = a.w_per_sample ? a.w[tl.b] : a.w[0];
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int e0 = (i * 256 + t) * 4;
      float o[4], u[4], r[4];
      const int cnt = load_slot(co + e0, tl.rem - e0, o);      // (out may alias an input: a thread reads its elements before it writes them)
      load_slot(un + e0, tl.rem - e0, u);
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = guidance_combine(a.guidance_cfg, o[k], u[k], w) * g;
      store_slot(out + e0, cnt, r);
    }
    // (no barrier here: thread 0 writes g_s, and the others red, only after the next pair's first barrier / after its second one)
  }
}

}  // namespace
}  // namespace pd

using namespace pd;

extern "C" size_t pd_guidance_rescale_workspace(int64_t B, int64_t n) {
  return (size_t)(n >= 2 ? chunks_of(B, n, CHUNK) * B : 0) * NSUM * sizeof(double);
}

extern "C" int pd_guidance_rescale(const pd_guidance_rescale_args* a, void* stream) {
  const char* const who = "pd_guidance_rescale";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->model_out != nullptr, PD_ERR_ARG, "%s: model_out is NULL", who);
  PD_CHECK(a->uncond_out != nullptr, PD_ERR_ARG, "%s: uncond_out is NULL (the rescale is defined for a guided prediction only)", who);
  PD_CHECK(a->w != nullptr, PD_ERR_ARG, "%s: guidance without weights (w is NULL)", who);
  PD_CHECK(a->out != nullptr, PD_ERR_ARG, "%s: out is NULL", who);
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "%s: null workspace (pd_guidance_rescale_workspace gives its size)", who);
  PD_CHECK(a->rescale >= 0.0f && a->rescale <= 1.0f, PD_ERR_ARG, "%s: rescale = %g (must lie in [0, 1])", who, (double)a->rescale);
  PD_CHECK(((uintptr_t)a->model_out % 16 == 0) && ((uintptr_t)a->uncond_out % 16 == 0) && ((uintptr_t)a->out % 16 == 0), PD_ERR_ARG,
           "%s: tensors must be 16-byte aligned", who);
  PD_CHECK((uintptr_t)a->w % 4 == 0, PD_ERR_ARG, "%s: w must be 4-byte aligned", who);
  PD_CHECK((uintptr_t)a->workspace % 8 == 0, PD_ERR_ARG, "%s: workspace must be 8-byte aligned", who);
  PD_CHECK(a->numel > 0, PD_ERR_SHAPE, "%s: numel = %lld (must be > 0)", who, (long long)a->numel);
  PD_CHECK(a->per_sample >= 2, PD_ERR_SHAPE, "%s: per_sample = %lld (a standard deviation takes at least two elements)", who,
           (long long)a->per_sample);
  PD_CHECK(a->numel % a->per_sample == 0, PD_ERR_SHAPE, "%s: numel %lld is not a multiple of per_sample %lld", who, (long long)a->numel,
           (long long)a->per_sample);
  Launch p;
  p.a = *a;
  const int64_t B = a->numel / a->per_sample;
  p.chunks = chunks_of(B, a->per_sample, CHUNK);
  PD_CHECK(p.chunks > 0, PD_ERR_SHAPE, "%s: more than 2^31 - 1 chunks of %d elements: split the batch", who, CHUNK);
  p.items = B * p.chunks;
  p.part = (double*)a->workspace;
  const unsigned grid = (unsigned)(p.items < MAX_BLOCKS ? p.items : MAX_BLOCKS);
  hipLaunchKernelGGL(guidance_rescale_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(guidance_rescale_apply_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
