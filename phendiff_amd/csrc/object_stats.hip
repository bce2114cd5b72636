// Per-object measurements: from the sparse labels of pd_mask_components (mask_morph.hip) to one table row per object.  Contract:
// include/phendiff_hip.h.  Host side: phendiff_amd.objects (label_objects, measure_intensity, ObjectMeasure, object_change,
// measure_transfer).  Labels and indices are dense int32 [B][H][W]; H, W <= PD_MASK_MAX_SIDE; K = max_objects table rows per sample.
//     pd_object_index      dense labels 1..count in raster order of the roots (scipy.ndimage.label's numbering), count, status   4 launches
//     pd_object_geometry   int64 [B][K][12]: area, bounding box, raw moments, edges, border                                      3 launches
//     pd_object_intensity  double [B][K][C][4]: sum, sum of squares, min, max of an image stack under the labels                 1 launch
//
// The house rules of mask_morph.hip and sample_stats.hip hold.  Integers are exact: the only atomics are INTEGER ones (64-bit add /
// min / max / or on a geometry row, a 32-bit or on a status word), whose result has no order.  Floating-point sums are fp64, added in
// an order the sizes fix, reduced in pd_reduce.h's fixed tree: no floating-point atomic.  A sample's result is a function of that sample alone
// (every index is formed within the sample; a pixel at a row's end is no neighbour of the next row's first pixel).  Everything is
// validated before the first launch; no host read, no allocation: capturable.  No loop is unbounded: every trip count below is a
// function of the sizes, or of a bounding box clamped to the image.
#include <limits.h>

#include "pd_reduce.h"

namespace pd {
namespace {

constexpr int MAX_SIDE = PD_MASK_MAX_SIDE, MAX_OBJECTS = PD_OBJ_MAX_OBJECTS, G = PD_OBJ_GEOM_FIELDS, NI = PD_OBJ_INTENSITY_FIELDS;
constexpr int TILE = 1024;                 // pixels per workgroup of the prefix sum: 4 consecutive pixels per thread
constexpr int64_t MAX_BLOCKS = 65536;      // more items than this many blocks take are walked in a grid-stride loop

static_assert((int64_t)MAX_SIDE * MAX_SIDE <= MAX_OBJECTS && MAX_OBJECTS == (1 << 28), "a sample holds at most 2^28 objects, and sum_yy < 2^56");

unsigned grid_of(int64_t items, int per_block) {
  const int64_t blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

#define PD_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- dense labels ----------------------------------------------------------------------------------------------------------------------
struct IndexLaunch {
  pd_object_index_args a;
  int hw;              // H * W <= 2^28
  int tiles;           // ceil(hw / TILE) <= 2^18
  int32_t* rank;       // [B][hw]: 1 + the number of roots before the pixel in its sample where the pixel is a root, else 0
  int32_t* tile_off;   // [B][tiles]: the tile's number of roots, then (scan) the number of roots before the tile
};

// The root flags of thread t's four pixels of the tile at j0 (pixels past the sample's end are no roots); returns their number.
__device__ __forceinline__ int tile_roots(const int32_t* lab, int j0, int hw, int t, int (&f)[4]) {
  int n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = j0 + 4 * t + k;
    f[k] = (j < hw && lab[j] == j + 1) ? 1 : 0;
    n += f[k];
  }
  return n;
}

// Exclusive prefix sum of n over the 256 threads in thread order, and the total: a wave scan of six shuffle steps, then the four wave
// totals through LDS.  Integer adds: exact in any order.  (The second barrier lets a caller's loop write `part` again.)
__device__ __forceinline__ int block_exclusive(int n, int* part, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = n;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d);
    if (lane >= d) inc += v;
  }
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) base += w < wave ? part[w] : 0;
  total = part[0] + part[1] + part[2] + part[3];
  __syncthreads();
  return base + inc - n;
}

__global__ __launch_bounds__(256) void index_count_kernel(const IndexLaunch p) {
  __shared__ int part[4];
  const int64_t items = p.a.B * p.tiles;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t s = item / p.tiles;
    const int j0 = (int)(item - s * p.tiles) * TILE;
    int f[4], total;
    block_exclusive(tile_roots(p.a.label + s * p.hw, j0, p.hw, threadIdx.x, f), part, total);
    if (threadIdx.x == 0) p.tile_off[item] = total;
  }
}

// One workgroup per sample: tile counts -> exclusive offsets, 256 tiles at a time with a carry (ceil(tiles / 256) <= 1024 steps).
__global__ __launch_bounds__(256) void index_scan_kernel(const IndexLaunch p) {
  __shared__ int part[4];
  const int t = threadIdx.x;
  for (int64_t s = blockIdx.x; s < p.a.B; s += gridDim.x) {
    int32_t* off = p.tile_off + s * p.tiles;
    int carry = 0;
    for (int base = 0; base < p.tiles; base += 256) {
      const bool in = base + t < p.tiles;
      int total;
      const int ex = block_exclusive(in ? off[base + t] : 0, part, total);
      if (in) off[base + t] = carry + ex;
      carry += total;
    }
    if (t == 0) {
      p.a.count[s] = carry;
      p.a.status[s] = (carry > p.a.max_objects ? PD_OBJ_OVERFLOW : 0) | (p.a.label_status && p.a.label_status[s] ? PD_OBJ_LABEL_STATUS : 0);
    }
  }
}

__global__ __launch_bounds__(256) void index_rank_kernel(const IndexLaunch p) {
  __shared__ int part[4];
  const int64_t items = p.a.B * p.tiles;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t s = item / p.tiles;
    const int j0 = (int)(item - s * p.tiles) * TILE;
    int f[4], total;
    const int n = tile_roots(p.a.label + s * p.hw, j0, p.hw, threadIdx.x, f);
    int r = p.tile_off[item] + block_exclusive(n, part, total) + 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + 4 * (int)threadIdx.x + k;
      if (j < p.hw) p.rank[s * p.hw + j] = f[k] ? r++ : 0;
    }
  }
}

// index = rank[label - 1] where that is a root of rank <= K.  A label that cannot be one (outside 1..hw, or naming a pixel that is no
// root) is never followed out of the sample's ranks: the pixel gets 0 and the sample's status word PD_OBJ_BAD_LABEL.
__global__ __launch_bounds__(256) void index_gather_kernel(const IndexLaunch p) {
  const int64_t numel = p.a.B * p.hw, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const int64_t s = i / p.hw;
    const int l = p.a.label[i];
    int idx = 0;
    if (l != 0) {
      const int r = (l >= 1 && l <= p.hw) ? p.rank[s * p.hw + l - 1] : 0;
      if (r == 0) atomicOr(p.a.status + s, PD_OBJ_BAD_LABEL);
      else if (r <= p.a.max_objects) idx = r;
    }
    p.a.index[i] = idx;
  }
}

// ---- geometry --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void geom_init_kernel(const pd_object_geometry_args a) {
  const int64_t numel = a.B * a.max_objects * G, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const int f = (int)(i % G);
    a.geometry[i] = (f == PD_OG_Y0 || f == PD_OG_X0) ? INT64_MAX : 0;
  }
}

// One wave per (sample, row, 64 columns).  A RUN is a maximal stretch of lanes with one index: contiguous pixels of one row, so the
// run's first lane knows everything but the edges in closed form -- its length from the ballot of the run starts, the x sums from the
// first x and the length -- and the edges come from a segmented wave sum.  Only a run's first lane issues atomics.  The loop's trip
// count is uniform over a wave (the item is the wave's), so the shuffles and the ballot see all 64 lanes.
__global__ __launch_bounds__(256) void geom_accum_kernel(const pd_object_geometry_args a, const int segs) {
  const int lane = threadIdx.x & 63, H = a.H, W = a.W, K = a.max_objects;
  const int64_t items = a.B * H * segs, waves = (int64_t)gridDim.x * 4;
  for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += waves) {
    const int64_t sy = item / segs;                       // s * H + y
    const int64_t s = sy / H;
    const int y = (int)(sy - s * H), x = (int)(item - sy * segs) * 64 + lane;
    const int32_t* ix = a.index + sy * W + x;             // (dereferenced only under x < W, its neighbours only inside the sample)
    int idx = -1, e = 0;                                  // -1: a lane past the row's end (a run of its own that is never emitted)
    if (x < W) {
      const unsigned v = (unsigned)ix[0];
      idx = v <= (unsigned)K ? (int)v : 0;                // an index outside 0..K is read as 0 (and differs from every object below)
      if (idx > 0) {
        e += !(x > 0 && ix[-1] == idx);
        e += !(x < W - 1 && ix[1] == idx);
        e += !(y > 0 && ix[-W] == idx);
        e += !(y < H - 1 && ix[W] == idx);
      }
    }
    const int prev = __shfl_up(idx, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != idx);
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);      // run starts in the lanes after this one
    const int n = after ? __ffsll((long long)after) : 64 - lane;                   // at a run's first lane: its length
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {      // e: the sum over lanes [lane, lane + 2 d) of the lane's run
      const int o = __shfl_down(e, d);
      if (lane + d < 64 && (after & ((1ull << d) - 1)) == 0) e += o;
    }
    if (idx > 0 && ((heads >> lane) & 1)) {
      unsigned long long* row = (unsigned long long*)(a.geometry + (s * K + (idx - 1)) * G);
      const unsigned long long n64 = (unsigned long long)n, x64 = (unsigned long long)x, y64 = (unsigned long long)y;
      const unsigned long long sx = n64 * x64 + n64 * (n64 - 1) / 2;
      const unsigned long long sxx = n64 * x64 * x64 + x64 * n64 * (n64 - 1) + (n64 - 1) * n64 * (2 * n64 - 1) / 6;
      const int x1 = x + n - 1;
      __hip_atomic_fetch_add(row + PD_OG_AREA, n64, PD_RLX);
      __hip_atomic_fetch_add(row + PD_OG_SUM_Y, y64 * n64, PD_RLX);
      __hip_atomic_fetch_add(row + PD_OG_SUM_X, sx, PD_RLX);
      __hip_atomic_fetch_add(row + PD_OG_SUM_YY, y64 * y64 * n64, PD_RLX);
      __hip_atomic_fetch_add(row + PD_OG_SUM_XX, sxx, PD_RLX);
      __hip_atomic_fetch_add(row + PD_OG_SUM_YX, y64 * sx, PD_RLX);
      __hip_atomic_fetch_add(row + PD_OG_EDGES, (unsigned long long)e, PD_RLX);
      __hip_atomic_fetch_min(row + PD_OG_Y0, y64, PD_RLX);
      __hip_atomic_fetch_max(row + PD_OG_Y1, y64, PD_RLX);
      __hip_atomic_fetch_min(row + PD_OG_X0, x64, PD_RLX);
      __hip_atomic_fetch_max(row + PD_OG_X1, (unsigned long long)x1, PD_RLX);
      if (y == 0 || y == H - 1 || x == 0 || x1 == W - 1) __hip_atomic_fetch_or(row + PD_OG_BORDER, 1ull, PD_RLX);
    }
  }
}

__global__ __launch_bounds__(256) void geom_final_kernel(const pd_object_geometry_args a) {
  const int64_t rows = a.B * a.max_objects, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += stride) {
    int64_t* row = a.geometry + i * G;
    if (row[PD_OG_AREA] == 0) row[PD_OG_Y0] = row[PD_OG_X0] = 0;
  }
}

// ---- intensity -------------------------------------------------------------------------------------------------------------------------
// One workgroup per (sample, table row, channel).  Thread t adds the selected pixels at box positions t, t + 256, ... in that order;
// the 256 partial results go through pd_reduce.h's workgroup reduction: the tree depends on the box alone.  Minimum and maximum are
// the compare-and-select forms, which never take a NaN: the flag says whether one was seen.
template <typename T>
__global__ __launch_bounds__(256) void intensity_kernel(const pd_object_intensity_args a) {
  using Vals = Ops<Sum, Sum, SelectMin, SelectMax>;      // sum, sum of squares, min, max
  __shared__ double red[4][4];
  __shared__ int flag[4][1];
  const int t = threadIdx.x, H = a.H, W = a.W, K = a.max_objects, Cn = a.C;
  const int64_t item = blockIdx.x;                        // (s * K + k - 1) * C + c
  const int64_t sk = item / Cn;
  const int c = (int)(item - sk * Cn);
  const int64_t s = sk / K;
  const int k = (int)(sk - s * K) + 1;
  const int64_t* g = a.geometry + sk * G;
  double* out = a.out + item * NI;
  if (g[PD_OG_AREA] <= 0) {                               // (uniform) an empty slot
    if (t < NI) out[t] = 0.0;
    return;
  }
  const int64_t gy0 = g[PD_OG_Y0], gy1 = g[PD_OG_Y1], gx0 = g[PD_OG_X0], gx1 = g[PD_OG_X1];
  const int y0 = (int)(gy0 < 0 ? 0 : gy0 > H - 1 ? H - 1 : gy0), y1 = (int)(gy1 < y0 ? y0 : gy1 > H - 1 ? H - 1 : gy1);
  const int x0 = (int)(gx0 < 0 ? 0 : gx0 > W - 1 ? W - 1 : gx0), x1 = (int)(gx1 < x0 ? x0 : gx1 > W - 1 ? W - 1 : gx1);
  const int bw = x1 - x0 + 1, n = (y1 - y0 + 1) * bw;     // <= H * W <= 2^28
  const int32_t* ix = a.index + s * H * W;
  const T* img = (const T*)a.images + (s * Cn + c) * H * W;
  double sum = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
  int seen = 0;                                           // bit 0: a pixel was selected; bit 1: one of them is a NaN
  for (int p = t; p < n; p += 256) {
    const int r = p / bw, j = (y0 + r) * W + x0 + (p - r * bw);
    if (ix[j] == k) {
      const double v = (double)img[j];
      sum += v;
      sq += v * v;
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
      seen |= v != v ? 3 : 1;
    }
  }
  double v[4] = {sum, sq, mn, mx};
  int all[1] = {seen};
  block_put(Vals(), v, red);
  block_put(Ops<Or>(), all, flag);
  __syncthreads();
  if (t == 0) {
    block_get(Vals(), v, red);
    block_get(Ops<Or>(), all, flag);
    if (all[0] & 2) v[2] = v[3] = __builtin_nan("");
    if (!(all[0] & 1)) v[2] = v[3] = 0.0;                 // (a table row that names no pixel of this index)
    out[PD_OI_SUM] = v[0];
    out[PD_OI_SUMSQ] = v[1];
    out[PD_OI_MIN] = v[2];
    out[PD_OI_MAX] = v[3];
  }
}

int validate_bhwk(int64_t B, int H, int W, int K, const char* who) {
  PD_CHECK(B >= 1, PD_ERR_SHAPE, "%s: B = %lld (must be >= 1)", who, (long long)B);
  PD_CHECK(H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE, PD_ERR_SHAPE, "%s: H x W = %d x %d (each side 1 to %d)", who, H, W, MAX_SIDE);
  PD_CHECK(B < (1ll << 60) / ((int64_t)H * W), PD_ERR_SHAPE, "%s: B * H * W = %lld * %d * %d does not fit 60 bits", who, (long long)B, H, W);
  PD_CHECK(K >= 1 && K <= MAX_OBJECTS, PD_ERR_SHAPE, "%s: max_objects = %d (1 to %d)", who, K, MAX_OBJECTS);
  PD_CHECK(B < (1ll << 50) / K, PD_ERR_SHAPE, "%s: B * max_objects = %lld * %d does not fit 50 bits", who, (long long)B, K);
  return PD_OK;
}

bool sizes_ok(int64_t B, int H, int W) {
  return B >= 1 && H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE && B < (1ll << 60) / ((int64_t)H * W);
}

}  // namespace
}  // namespace pd

using namespace pd;

extern "C" size_t pd_object_index_workspace(int64_t B, int H, int W) {
  if (!sizes_ok(B, H, W)) return 0;
  const int64_t hw = (int64_t)H * W;
  return (size_t)(B * (hw + (hw + TILE - 1) / TILE)) * sizeof(int32_t);
}

extern "C" int pd_object_index(const pd_object_index_args* a, void* stream) {
  const char* const who = "pd_object_index";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->label != nullptr, PD_ERR_ARG, "%s: label is NULL", who);
  PD_CHECK(a->index != nullptr && a->count != nullptr && a->status != nullptr, PD_ERR_ARG, "%s: index / count / status is NULL", who);
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "%s: null workspace (pd_object_index_workspace gives its size)", who);
  PD_CHECK((uintptr_t)a->label % 4 == 0 && (uintptr_t)a->label_status % 4 == 0 && (uintptr_t)a->index % 4 == 0 && (uintptr_t)a->count % 4 == 0 &&
               (uintptr_t)a->status % 4 == 0 && (uintptr_t)a->workspace % 4 == 0,
           PD_ERR_ARG, "%s: label, label_status, index, count, status and workspace must be 4-byte aligned", who);
  if (const int rc = validate_bhwk(a->B, a->H, a->W, a->max_objects, who)) return rc;
  IndexLaunch p;
  p.a = *a;
  p.hw = a->H * a->W;
  p.tiles = (p.hw + TILE - 1) / TILE;
  p.rank = (int32_t*)a->workspace;
  p.tile_off = p.rank + a->B * p.hw;
  const int64_t items = a->B * p.tiles;
  const unsigned tile_grid = (unsigned)(items < MAX_BLOCKS ? items : MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(index_count_kernel, dim3(tile_grid), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(index_scan_kernel, dim3((unsigned)(a->B < MAX_BLOCKS ? a->B : MAX_BLOCKS)), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(index_rank_kernel, dim3(tile_grid), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(index_gather_kernel, dim3(grid_of(a->B * p.hw, 256)), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_object_geometry(const pd_object_geometry_args* a, void* stream) {
  const char* const who = "pd_object_geometry";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->index != nullptr, PD_ERR_ARG, "%s: index is NULL", who);
  PD_CHECK(a->geometry != nullptr, PD_ERR_ARG, "%s: geometry is NULL", who);
  PD_CHECK((uintptr_t)a->index % 4 == 0, PD_ERR_ARG, "%s: index must be 4-byte aligned", who);
  PD_CHECK((uintptr_t)a->geometry % 8 == 0, PD_ERR_ARG, "%s: geometry must be 8-byte aligned", who);
  if (const int rc = validate_bhwk(a->B, a->H, a->W, a->max_objects, who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = a->B * a->max_objects;
  hipLaunchKernelGGL(geom_init_kernel, dim3(grid_of(rows * G, 256)), dim3(256), 0, st, *a);
  PD_LAUNCH_CHECK();
  const int segs = (a->W + 63) / 64;
  hipLaunchKernelGGL(geom_accum_kernel, dim3(grid_of(a->B * a->H * segs, 4)), dim3(256), 0, st, *a, segs);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(geom_final_kernel, dim3(grid_of(rows, 256)), dim3(256), 0, st, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_object_intensity(const pd_object_intensity_args* a, void* stream) {
  const char* const who = "pd_object_intensity";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->index != nullptr && a->geometry != nullptr, PD_ERR_ARG, "%s: index / geometry is NULL (pd_object_index and pd_object_geometry write them)", who);
  PD_CHECK(a->images != nullptr, PD_ERR_ARG, "%s: images is NULL", who);
  PD_CHECK(a->out != nullptr, PD_ERR_ARG, "%s: out is NULL", who);
  PD_CHECK((uintptr_t)a->index % 4 == 0 && (uintptr_t)a->geometry % 8 == 0 && (uintptr_t)a->out % 8 == 0, PD_ERR_ARG,
           "%s: index must be 4-byte, geometry and out 8-byte aligned", who);
  if (const int rc = validate_bhwk(a->B, a->H, a->W, a->max_objects, who)) return rc;
  PD_CHECK(a->C >= 1, PD_ERR_SHAPE, "%s: C = %d (must be >= 1)", who, a->C);
  PD_CHECK(a->dtype == PD_OBJ_F32 || a->dtype == PD_OBJ_U8 || a->dtype == PD_OBJ_U16, PD_ERR_SHAPE, "%s: dtype = %d (PD_OBJ_F32, PD_OBJ_U8 or PD_OBJ_U16)", who,
           a->dtype);
  const int esz = a->dtype == PD_OBJ_F32 ? 4 : a->dtype == PD_OBJ_U16 ? 2 : 1;
  PD_CHECK((uintptr_t)a->images % esz == 0, PD_ERR_ARG, "%s: images must be aligned to their element (%d bytes)", who, esz);
  PD_CHECK(a->B * a->max_objects <= (int64_t)INT_MAX / a->C, PD_ERR_SHAPE, "%s: B * max_objects * C = %lld * %d * %d workgroups (at most 2^31 - 1)", who,
           (long long)a->B, a->max_objects, a->C);
  PD_CHECK(a->B * a->C < (1ll << 60) / ((int64_t)a->H * a->W), PD_ERR_SHAPE, "%s: B * C * H * W does not fit 60 bits", who);
  const dim3 grid((unsigned)(a->B * a->max_objects * a->C));
  hipStream_t st = (hipStream_t)stream;
  if (a->dtype == PD_OBJ_F32) hipLaunchKernelGGL(intensity_kernel<float>, grid, dim3(256), 0, st, *a);
  else if (a->dtype == PD_OBJ_U8) hipLaunchKernelGGL(intensity_kernel<uint8_t>, grid, dim3(256), 0, st, *a);
  else hipLaunchKernelGGL(intensity_kernel<uint16_t>, grid, dim3(256), 0, st, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
