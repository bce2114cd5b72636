// pd_sample_stats: per-sample diagnostics of a [B][n] tensor without a trip to the host -- sum / min / max / non-finite count, the central
// moments m2 m3 m4 about the fp64 mean, a histogram over caller-given edges and, against an optional second tensor, the L1 / squared / max
// error.  What check_Gaussianity (utils_Img2Img.py:79-93) and Lp_loss (:245-270) compute on the host.  Contract: include/phendiff_hip.h.
//
// Five launches on one stream, no host synchronisation: [zero hist] -> pass A (per-chunk sum / min / max / non-finite) -> fold A (the
// sample's sum, hence its mean) -> pass B (per-chunk sums of d^2 d^3 d^4 with d = x - mean, the error sums, the histogram) -> fold B.
// A sample is tiled into chunks of PD_SAMPLE_STATS_CHUNK elements, one workgroup of 256 threads per (sample, chunk).
//
// Determinism: every floating-point reduction runs in the one fixed order of pd_reduce.h.  Which element a lane takes depends only on the
// element's index WITHIN ITS SAMPLE, never on the address (load_slot), so a sample's results do not depend on B, on its row in the batch
// or on its alignment.  The histogram uses integer atomics only (LDS, then one global add per non-empty bin and workgroup):
// order-independent.  No float atomics.
#include "pd_reduce.h"
#include "pd_step.h"      // Slot, load_slot

namespace pd {
namespace {

constexpr int CHUNK = PD_SAMPLE_STATS_CHUNK, MAX_BINS = PD_SAMPLE_STATS_MAX_BINS, F = PD_SAMPLE_STATS_FIELDS;

// ---- the two sets of per-chunk partials and how each member combines (fmin / fmax: a NaN operand loses)
template <int PASS> struct Part;
template <> struct Part<0> : Ops<Sum, Fmin, Fmax, Sum> {};                // sum, min, max, non-finite count
template <> struct Part<1> : Ops<Sum, Sum, Sum, Sum, Sum, Fmax> {};       // sum d^2, sum d^3, sum d^4, sum |e|, sum e^2, max |e|

// lane -> wave -> workgroup; thread 0 writes the N results to out
template <int PASS> __device__ __forceinline__ void block_reduce_to(double (&acc)[Part<PASS>::N], double (*red)[Part<PASS>::N], double* out) {
  block_reduce(Part<PASS>(), acc, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < Part<PASS>::N; ++i) out[i] = acc[i];
  }
}

struct Launch {
  pd_sample_stats_args a;
  int64_t chunks;        // per sample
  double* part[2];       // [B][chunks][Part<PASS>::N]
};

__global__ __launch_bounds__(256) void zero_u32_kernel(uint32_t* p, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) p[i] = 0u;
}

template <typename T> __global__ __launch_bounds__(256) void pass_a_kernel(const Launch p) {
  constexpr int VEC = Slot<T>::VEC, ITERS = CHUNK / (256 * VEC);
  __shared__ double red[4][Part<0>::N];
  const int64_t blk = blockIdx.x;
  const ChunkTile tl = chunk_tile(blk, p.chunks, p.a.n, CHUNK);
  const int64_t b = tl.b, j0 = tl.j0;
  const int rem = tl.rem;
  const T* x = (const T*)p.a.x + b * p.a.n + j0;
  double acc[4] = {0.0, (double)INFINITY, -(double)INFINITY, 0.0};
  uint32_t bad = 0;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int e0 = (i * 256 + (int)threadIdx.x) * VEC;
    float v[VEC];
    const int cnt = load_slot<T>(x + e0, rem - e0, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (k < cnt) {
        const double d = (double)v[k];
        acc[0] += d;
        acc[1] = fmin(acc[1], d);      // (fmin / fmax pass over a NaN: min and max are those of the other elements)
        acc[2] = fmax(acc[2], d);
        bad += __builtin_isfinite(v[k]) ? 0u : 1u;
      }
    }
  }
  acc[3] = (double)bad;
  block_reduce_to<0>(acc, red, p.part[0] + blk * Part<0>::N);
}

// one workgroup per sample folds its chunks' partials
template <int PASS> __global__ __launch_bounds__(256) void fold_kernel(const Launch p) {
  constexpr int N = Part<PASS>::N;
  __shared__ double red[256][N];
  const int64_t b = blockIdx.x;
  double r[N];
  run_fold(Part<PASS>(), p.part[PASS] + b * p.chunks * N, p.chunks, red, r);
  if (threadIdx.x != 0) return;
  double* st = p.a.stats + b * F;
  if (PASS == 0) {
    st[PD_SS_SUM] = r[0]; st[PD_SS_MIN] = r[1]; st[PD_SS_MAX] = r[2]; st[PD_SS_NONFINITE] = r[3];
  } else {
    const double n = (double)p.a.n;
    st[PD_SS_M2] = r[0] / n; st[PD_SS_M3] = r[1] / n; st[PD_SS_M4] = r[2] / n;
    st[PD_SS_ERR_L1] = r[3]; st[PD_SS_ERR_SQ] = r[4]; st[PD_SS_ERR_MAX] = r[5];
  }
}

template <typename T> __global__ __launch_bounds__(256) void pass_b_kernel(const Launch p) {
  constexpr int VEC = Slot<T>::VEC, ITERS = CHUNK / (256 * VEC);
  extern __shared__ double dyn[];      // bins > 0: edges [bins + 1] (fp64), then the workgroup's histogram [bins] (uint32)
  __shared__ double red[4][Part<1>::N];
  const int bins = p.a.bins, t = threadIdx.x;
  double* edges = dyn;
  uint32_t* lh = (uint32_t*)(dyn + bins + 1);
  if (bins > 0) {
    for (int i = t; i <= bins; i += 256) edges[i] = p.a.edges[i];
    for (int i = t; i < bins; i += 256) lh[i] = 0u;
    __syncthreads();
  }
  const int64_t blk = blockIdx.x;
  const ChunkTile tl = chunk_tile(blk, p.chunks, p.a.n, CHUNK);
  const int64_t b = tl.b, j0 = tl.j0;
  const int rem = tl.rem;
  const T* x = (const T*)p.a.x + b * p.a.n + j0;
  const T* y = p.a.y ? (const T*)p.a.y + b * p.a.y_sample_stride + j0 : nullptr;
  const double mean = p.a.stats[b * F + PD_SS_SUM] / (double)p.a.n;
  const double lo = bins > 0 ? edges[0] : 0.0, hi = bins > 0 ? edges[bins] : 0.0;
  const double scale = (double)bins / (hi - lo);
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int e0 = (i * 256 + t) * VEC;
    float v[VEC], w[VEC];
    const int cnt = load_slot<T>(x + e0, rem - e0, v);
    if (y) load_slot<T>(y + e0, rem - e0, w);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (k < cnt) {
        const double xv = (double)v[k], d = xv - mean, d2 = d * d;
        acc[0] += d2;
        acc[1] += d2 * d;
        acc[2] += d2 * d2;
        if (y) {
          const double e = xv - (double)w[k], ae = fabs(e);
          acc[3] += ae;
          acc[4] += e * e;
          acc[5] = fmax(acc[5], ae);
        }
        if (bins > 0 && xv >= lo && xv <= hi) {      // (a NaN fails both comparisons)
          // the guess from fp64 arithmetic can be one off at an edge: the comparisons with the edges decide
          int g = (int)((xv - lo) * scale);
          g = g < 0 ? 0 : (g > bins - 1 ? bins - 1 : g);
          while (g > 0 && xv < edges[g]) --g;
          while (g < bins - 1 && xv >= edges[g + 1]) ++g;
          if (xv >= edges[g] && (xv < edges[g + 1] || g == bins - 1)) atomicAdd(&lh[g], 1u);
        }
      }
    }
  }
  block_reduce_to<1>(acc, red, p.part[1] + blk * Part<1>::N);      // (its barrier also closes the LDS histogram)
  if (bins > 0) {
    uint32_t* out = p.a.hist + b * bins;
    for (int i = t; i < bins; i += 256) {
      const uint32_t h = lh[i];
      if (h) atomicAdd(out + i, h);
    }
  }
}

template <typename T> int launch_all(const Launch& p, hipStream_t st) {
  const pd_sample_stats_args& a = p.a;
  const unsigned grid = (unsigned)(a.B * p.chunks);
  const size_t lds = a.bins > 0 ? (size_t)(a.bins + 1) * 8 + (size_t)a.bins * 4 : 0;
  if (a.bins > 0) {
    const int64_t count = a.B * a.bins, blocks = (count + 255) / 256;
    hipLaunchKernelGGL(zero_u32_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, a.hist, count);
    PD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pass_a_kernel<T>, dim3(grid), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(fold_kernel<0>, dim3((unsigned)a.B), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(pass_b_kernel<T>, dim3(grid), dim3(256), lds, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(fold_kernel<1>, dim3((unsigned)a.B), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // namespace
}  // namespace pd

extern "C" size_t pd_sample_stats_workspace(int64_t B, int64_t n, int bins) {
  using namespace pd;
  if (bins < 0 || bins > MAX_BINS) return 0;
  return (size_t)(B > 0 && n > 0 ? chunks_of(B, n, CHUNK) * B : 0) * (Part<0>::N + Part<1>::N) * sizeof(double);
}

extern "C" int pd_sample_stats(const pd_sample_stats_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_sample_stats: null args");
  PD_CHECK(a->x != nullptr, PD_ERR_ARG, "pd_sample_stats: null x");
  PD_CHECK(a->stats != nullptr, PD_ERR_ARG, "pd_sample_stats: null stats output");
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "pd_sample_stats: null workspace (pd_sample_stats_workspace gives its size)");
  PD_CHECK(a->dtype == PD_F32 || a->dtype == PD_BF16 || a->dtype == PD_F16, PD_ERR_ARG, "pd_sample_stats: dtype %d (PD_F32 / PD_BF16 / PD_F16)", a->dtype);
  PD_CHECK(a->bins >= 0, PD_ERR_ARG, "pd_sample_stats: bins = %d (must not be negative)", a->bins);
  PD_CHECK(a->bins == 0 || a->edges != nullptr, PD_ERR_ARG, "pd_sample_stats: bins = %d without edges", a->bins);
  PD_CHECK(a->bins == 0 || a->hist != nullptr, PD_ERR_ARG, "pd_sample_stats: bins = %d without a hist output", a->bins);
  PD_CHECK(a->B > 0 && a->n > 0, PD_ERR_SHAPE, "pd_sample_stats: B and n must be positive");
  PD_CHECK(a->bins <= MAX_BINS, PD_ERR_SHAPE, "pd_sample_stats: bins = %d above the LDS histogram's %d", a->bins, MAX_BINS);
  PD_CHECK(a->y == nullptr || a->y_sample_stride == 0 || a->y_sample_stride == a->n, PD_ERR_SHAPE,
           "pd_sample_stats: y_sample_stride %lld (n = %lld for one y per sample, 0 to broadcast one)", (long long)a->y_sample_stride, (long long)a->n);
  PD_CHECK(a->B < (1ll << 31) && a->n < (1ll << 62) / a->B, PD_ERR_SHAPE, "pd_sample_stats: B * n must stay below 2^62");
  PD_CHECK(a->bins == 0 || a->n < (1ll << 32), PD_ERR_SHAPE, "pd_sample_stats: n must stay below 2^32 with a histogram (uint32 counts)");
  Launch p;
  p.a = *a;
  p.chunks = chunks_of(a->B, a->n, CHUNK);
  PD_CHECK(p.chunks > 0, PD_ERR_SHAPE, "pd_sample_stats: grid too large (more than 2^31 - 1 blocks of %d elements): split the batch", CHUNK);
  const size_t need = (size_t)(p.chunks * a->B) * (Part<0>::N + Part<1>::N) * sizeof(double);
  PD_CHECK(a->workspace_bytes >= need, PD_ERR_ARG, "pd_sample_stats: workspace_bytes %zu below the %zu that pd_sample_stats_workspace asks for",
           a->workspace_bytes, need);
  p.part[0] = (double*)a->workspace;
  p.part[1] = p.part[0] + p.chunks * a->B * Part<0>::N;
  switch (a->dtype) {
    case PD_F32: return launch_all<float>(p, (hipStream_t)stream);
    case PD_BF16: return launch_all<bf16_t>(p, (hipStream_t)stream);
    default: return launch_all<half_t>(p, (hipStream_t)stream);
  }
}
