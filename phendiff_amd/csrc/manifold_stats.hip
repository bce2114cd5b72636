// pd_knn_radii / pd_manifold_query: the k-nearest-neighbour manifold estimates under improved precision / recall (Kynkaanniemi et al.
// 2019) and density / coverage (Naeem et al. 2020), in fp64 over fp32 features that stay on the device.  Contract: include/phendiff_hip.h.
//
// Everything is in SQUARED distances, d2(a, b) = max(0, |a|^2 + |b|^2 - 2 a.b), NaN -> +inf.  The dot products are 64 x 64 Gram tiles on
// v_mfma_f64_16x16x4_f64, the engine of metric_stats.hip's kid_tile_kernel (fp32 rows staged through LDS, KC = 32 columns at a time, widened
// exactly on the way to the MFMA; operand maps as stated there).  The norms come from the SAME instruction sequence: norm_kernel feeds a
// block of 16 rows to the MFMA as both operands, 16 columns per step in the tile kernels' order, and keeps the diagonal -- so |a|^2 is
// bit for bit the Gram entry of a with itself, and two bitwise-equal rows are at distance exactly 0.
//
//   pd_knn_radii        norms; then one workgroup (4 waves, 2 x 2, each 32 x 32) per (block of 64 rows, split of the column tiles).  After
//                       each tile the d2 values go through LDS to 4 threads per row, each of which keeps the KT smallest of its 16 columns
//                       in a sorted register list (a statically unrolled compare-swap chain; KT = 4, 8 or 17 >= k + 1).  The four lists
//                       of a row are merged through LDS and the k + 1 smallest go to the workspace; a second launch merges the splits.
//   pd_manifold_query   norms of both sides; the same walk with queries as rows and references as columns; a lane keeps a count and a
//                       minimum for each of its 8 rows, reduced over the 16 lanes of a row by xor shuffles, over the 2 waves through LDS,
//                       over the splits by a second launch.
//
// Determinism: no atomics.  A pair's d2 is a function of its two rows alone (one fixed MFMA sequence over D whatever the tile, the split or
// the batch), and the reductions are order statistics, integer sums and minima: the outputs do not depend on `splits` or on the order of the
// rows, bit for bit.  Rows at or past N of a ragged tile are not read (zeros are staged) and their d2 is SELECTED to +inf, never multiplied
// by zero; the diagonal of pd_knn_radii is selected to 0.
#include <math.h>
#include "pd_common.h"

namespace pd {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 64;                        // 64 x 64 distances per step of a workgroup
constexpr int KC = 32, LDP = KC + 4;            // fp32 columns staged per step; LDS row pitch in floats (144 bytes: 16-byte aligned rows)
constexpr int DP = TILE + 1;                    // pitch of the d2 tile in doubles
constexpr int KMAX1 = PD_MANIFOLD_MAX_K + 1;
// the default `splits` aims at this many workgroups: 16 rounds of two per CU on 256 CUs, so the last, partly idle round costs little.  A tuning
// value, private to this file: callers learn the default from the workspace queries (docs/LAB_r22.md has the measurement behind it)
constexpr int TARGET_GROUPS = 8192;

bool width_ok(int D) { return D >= 64 && D <= 4096 && D % 64 == 0; }

// splits in effect (0: the default, from the shapes only), or -1 where refused
int resolve_splits(int64_t rows, int64_t cols, int splits) {
  if (splits < 0 || splits > PD_MANIFOLD_MAX_SPLITS || rows < 1 || cols < 1) return -1;
  if (splits > 0) return splits;
  const int64_t rb = (rows + TILE - 1) / TILE, nct = (cols + TILE - 1) / TILE;
  int64_t s = (TARGET_GROUPS + rb - 1) / rb;
  if (s > nct) s = nct;
  if (s > PD_MANIFOLD_MAX_SPLITS) s = PD_MANIFOLD_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

__device__ __forceinline__ double dist2(double na, double nb, double dot) {
  const double v = (na + nb) - 2.0 * dot;
  return v > 0.0 ? v : (v <= 0.0 ? 0.0 : INFINITY);      // NaN -> +inf
}

// sorted (ascending) list of the KT smallest values seen: v bubbles through, the largest falls off the end
template <int KT> __device__ __forceinline__ void insert(double (&l)[KT], double v) {
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const bool lt = v < l[i];
    const double lo = lt ? v : l[i], hi = lt ? l[i] : v;
    l[i] = lo;
    v = hi;
  }
}

// |row|^2 of 16 rows per wave, by the tile kernels' MFMA sequence with the block as both operands (the diagonal of its Gram matrix)
__global__ __launch_bounds__(256) void norm_kernel(const float* __restrict__ f, int64_t stride, int64_t N, int D, double* __restrict__ out) {
  const int t = threadIdx.x, lane = t & 63, r16 = lane & 15, g = lane >> 4;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (t >> 6)) * 16 + r16;
  const float* p = row < N ? f + row * stride + g * 4 : nullptr;
  f64x4 acc = (f64x4)(0.0);
  for (int k = 0; k < D; k += 16) {
    const f32x4 v = p ? *(const f32x4*)(p + k) : (f32x4)(0.f);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)v[q], (double)v[q], acc, 0, 0, 0);
  }
  // a lane holds C[g + 4 reg][r16]: the diagonal element of row r16 is in lane g = r16 & 3, register r16 >> 2
  double d = acc[0];
#pragma unroll
  for (int reg = 1; reg < 4; ++reg) d = (r16 >> 2) == reg ? acc[reg] : d;
  if (p && g == (r16 & 3)) out[row] = d;
}

// acc[i][j] = the 2 x 2 blocks of 16 x 16 dot products of this wave's 32 x 32 quarter of the tile; pa / pb: the loader's two rows of
// either operand at column 4 (t & 7), null for a row that does not exist
__device__ __forceinline__ void gram_tile(const float* const (&pa)[2], const float* const (&pb)[2], int D, float* sa, float* sb, f64x4 (&acc)[2][2]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r16 = lane & 15, g = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const int lrow = t >> 3, lc = (t & 7) * 4;
  f32x4 va[2], vb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      va[h] = pa[h] ? *(const f32x4*)(pa[h] + k0) : (f32x4)(0.f);
      vb[h] = pb[h] ? *(const f32x4*)(pb[h] + k0) : (f32x4)(0.f);
    }
  };
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4)(0.0);
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += KC) {
    __syncthreads();      // the previous step's reads are done
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *(f32x4*)&sa[(lrow + 32 * h) * LDP + lc] = va[h];
      *(f32x4*)&sb[(lrow + 32 * h) * LDP + lc] = vb[h];
    }
    __syncthreads();
    if (k0 + KC < D) fetch(k0 + KC);
#pragma unroll
    for (int kb = 0; kb < KC / 16; ++kb) {
      f32x4 fa4[2], fb4[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa4[i] = *(const f32x4*)&sa[(wr * 32 + i * 16 + r16) * LDP + kb * 16 + g * 4];
        fb4[i] = *(const f32x4*)&sb[(wc * 32 + i * 16 + r16) * LDP + kb * 16 + g * 4];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fa4[i][q], (double)fb4[j][q], acc[i][j], 0, 0, 0);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- pd_knn_radii
struct RadLaunch {
  pd_knn_radii_args a;
  int splits, nct;      // splits in effect; column tiles
  double* norm;         // [N]
  double* cand;         // [N][splits][k + 1], ascending
};

template <int KT> __global__ __launch_bounds__(256) void radii_tile_kernel(const RadLaunch p) {
  __shared__ __attribute__((aligned(16))) float sa[TILE * LDP];
  __shared__ __attribute__((aligned(16))) float sb[TILE * LDP];
  constexpr int SD = 256 * KT > TILE * DP ? 256 * KT : TILE * DP;
  __shared__ double sd[SD];             // the d2 tile; at the end the four lists of every row
  const pd_knn_radii_args& a = p.a;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r16 = lane & 15, g = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const int64_t rb = (int64_t)blockIdx.x / p.splits;
  const int s = (int)((int64_t)blockIdx.x - rb * p.splits);
  const int ct0 = (int)((int64_t)s * p.nct / p.splits), ct1 = (int)((int64_t)(s + 1) * p.nct / p.splits);
  const int lrow = t >> 3, lc = (t & 7) * 4;
  const float* pa[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t ra = rb * TILE + lrow + 32 * h;
    pa[h] = ra < a.N ? a.f + ra * a.f_stride + lc : nullptr;
  }
  double na[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t gi = rb * TILE + wr * 32 + i * 16 + g + 4 * reg;
      na[i][reg] = gi < a.N ? p.norm[gi] : 0.0;
    }
  const int srow = t >> 2, part = t & 3;      // the selection: 4 threads per row, 16 columns each
  double lst[KT];
#pragma unroll
  for (int i = 0; i < KT; ++i) lst[i] = INFINITY;
  for (int ct = ct0; ct < ct1; ++ct) {
    const float* pb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t rc = (int64_t)ct * TILE + lrow + 32 * h;
      pb[h] = rc < a.N ? a.f + rc * a.f_stride + lc : nullptr;
    }
    f64x4 acc[2][2];
    gram_tile(pa, pb, a.D, sa, sb, acc);
    __syncthreads();      // the previous tile's reads of sd are done (one barrier per 64 x 64 x D tile; not left to gram_tile's own)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t gj = (int64_t)ct * TILE + wc * 32 + j * 16 + r16;
      const bool col = gj < a.N;
      const double nb = col ? p.norm[gj] : 0.0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int li = wr * 32 + i * 16 + g + 4 * reg;
          double v = dist2(na[i][reg], nb, acc[i][j][reg]);
          v = col ? v : INFINITY;
          v = rb * TILE + li == gj ? 0.0 : v;      // the row's own entry: exactly 0, not computed
          sd[li * DP + wc * 32 + j * 16 + r16] = v;
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < 16; ++c) {
      const double v = sd[srow * DP + part * 16 + c];
      if (v < lst[KT - 1]) insert<KT>(lst, v);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < KT; ++i) sd[t * KT + i] = lst[i];
  __syncthreads();
  const int64_t grow = rb * TILE + srow;
  if (part == 0 && grow < a.N) {
    for (int o = 1; o < 4; ++o)
      for (int i = 0; i < KT; ++i) {
        const double v = sd[(t + o) * KT + i];
        if (v < lst[KT - 1]) insert<KT>(lst, v);
      }
    double* out = p.cand + (grow * p.splits + s) * (a.k + 1);
#pragma unroll
    for (int i = 0; i < KT; ++i)
      if (i <= a.k) out[i] = lst[i];
  }
}

// one thread per row: the k + 1 smallest of the splits' candidates; rad2 = the largest of them
__global__ __launch_bounds__(256) void radii_merge_kernel(const RadLaunch p) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= p.a.N) return;
  double lst[KMAX1];
#pragma unroll
  for (int i = 0; i < KMAX1; ++i) lst[i] = INFINITY;
  const double* in = p.cand + row * p.splits * (p.a.k + 1);
  const int n = p.splits * (p.a.k + 1);
  for (int c = 0; c < n; ++c) {
    const double v = in[c];
    if (v < lst[KMAX1 - 1]) insert<KMAX1>(lst, v);
  }
  double r = lst[0];
#pragma unroll
  for (int i = 1; i < KMAX1; ++i) r = i == p.a.k ? lst[i] : r;
  p.a.rad2[row] = r;
}

// ---------------------------------------------------------------------------------------------------------------- pd_manifold_query
struct QryLaunch {
  pd_manifold_query_args a;
  int splits, nct;
  double* nq;           // [Nq]
  double* nr;           // [Nr]
  double* pmin;         // [Nq][splits]
  int32_t* pcnt;        // [Nq][splits]
};

__global__ __launch_bounds__(256) void query_tile_kernel(const QryLaunch p) {
  __shared__ __attribute__((aligned(16))) float sa[TILE * LDP];
  __shared__ __attribute__((aligned(16))) float sb[TILE * LDP];
  __shared__ double rmin[2][TILE];
  __shared__ int32_t rcnt[2][TILE];
  const pd_manifold_query_args& a = p.a;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r16 = lane & 15, g = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const int64_t rb = (int64_t)blockIdx.x / p.splits;
  const int s = (int)((int64_t)blockIdx.x - rb * p.splits);
  const int ct0 = (int)((int64_t)s * p.nct / p.splits), ct1 = (int)((int64_t)(s + 1) * p.nct / p.splits);
  const int lrow = t >> 3, lc = (t & 7) * 4;
  const bool counting = a.count != nullptr;
  const float* pa[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t ra = rb * TILE + lrow + 32 * h;
    pa[h] = ra < a.Nq ? a.q + ra * a.q_stride + lc : nullptr;
  }
  double na[2][4], mn[2][4];
  int32_t cnt[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t gi = rb * TILE + wr * 32 + i * 16 + g + 4 * reg;
      na[i][reg] = gi < a.Nq ? p.nq[gi] : 0.0;
      mn[i][reg] = INFINITY;
      cnt[i][reg] = 0;
    }
  for (int ct = ct0; ct < ct1; ++ct) {
    const float* pb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t rc = (int64_t)ct * TILE + lrow + 32 * h;
      pb[h] = rc < a.Nr ? a.r + rc * a.r_stride + lc : nullptr;
    }
    f64x4 acc[2][2];
    gram_tile(pa, pb, a.D, sa, sb, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t gj = (int64_t)ct * TILE + wc * 32 + j * 16 + r16;
      const bool col = gj < a.Nr;
      const double nb = col ? p.nr[gj] : 0.0;
      const double rd = counting && col ? a.rad2[gj] : -1.0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          double v = dist2(na[i][reg], nb, acc[i][j][reg]);
          v = col ? v : INFINITY;
          cnt[i][reg] += (v < INFINITY && v <= rd) ? 1 : 0;      // an infinite (NaN) distance is never counted, whatever the radius
          mn[i][reg] = v < mn[i][reg] ? v : mn[i][reg];
        }
    }
  }
  // over the 16 lanes that share a row (integer sums and minima: any order gives the same bits), then over the two waves of a row block
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
      for (int m = 8; m >= 1; m >>= 1) {
        const double o = __shfl_xor(mn[i][reg], m);
        mn[i][reg] = o < mn[i][reg] ? o : mn[i][reg];
        cnt[i][reg] += __shfl_xor(cnt[i][reg], m);
      }
      if (r16 == 0) {
        const int li = wr * 32 + i * 16 + g + 4 * reg;
        rmin[wc][li] = mn[i][reg];
        rcnt[wc][li] = cnt[i][reg];
      }
    }
  __syncthreads();
  const int64_t grow = rb * TILE + t;
  if (t < TILE && grow < a.Nq) {
    p.pmin[grow * p.splits + s] = rmin[1][t] < rmin[0][t] ? rmin[1][t] : rmin[0][t];
    p.pcnt[grow * p.splits + s] = rcnt[0][t] + rcnt[1][t];
  }
}

__global__ __launch_bounds__(256) void query_merge_kernel(const QryLaunch p) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= p.a.Nq) return;
  double mn = INFINITY;
  int32_t cnt = 0;
  for (int s = 0; s < p.splits; ++s) {
    const double v = p.pmin[row * p.splits + s];
    mn = v < mn ? v : mn;
    cnt += p.pcnt[row * p.splits + s];
  }
  if (p.a.count) p.a.count[row] = cnt;
  if (p.a.dmin2) p.a.dmin2[row] = mn;
}

bool rows_ok(int64_t n) { return n >= 1 && n < (1ll << 31); }

// bytes, or 0 where the sizes are refused
size_t radii_workspace(int64_t N, int k, int splits) {
  if (!rows_ok(N) || k < 1 || k > PD_MANIFOLD_MAX_K || k + 1 > N) return 0;
  const int s = resolve_splits(N, N, splits);
  if (s < 1) return 0;
  return (size_t)(N + N * s * (k + 1)) * sizeof(double);
}

size_t query_workspace(int64_t Nq, int64_t Nr, int splits) {
  if (!rows_ok(Nq) || !rows_ok(Nr)) return 0;
  const int s = resolve_splits(Nq, Nr, splits);
  if (s < 1) return 0;
  return (size_t)(Nq + Nr + Nq * s) * sizeof(double) + (((size_t)(Nq * s) * sizeof(int32_t) + 7) & ~(size_t)7);
}

}  // namespace
}  // namespace pd

extern "C" size_t pd_knn_radii_workspace(int64_t N, int k, int splits) { return pd::radii_workspace(N, k, splits); }

extern "C" int pd_knn_radii(const pd_knn_radii_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_knn_radii: null args");
  PD_CHECK(a->f != nullptr, PD_ERR_ARG, "pd_knn_radii: null features (f)");
  PD_CHECK(a->rad2 != nullptr, PD_ERR_ARG, "pd_knn_radii: null output (rad2)");
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "pd_knn_radii: null workspace (pd_knn_radii_workspace gives its size)");
  PD_CHECK(width_ok(a->D), PD_ERR_SHAPE, "pd_knn_radii: D = %d (a multiple of 64 in 64 .. 4096)", a->D);
  PD_CHECK(a->f_stride >= a->D && a->f_stride % 4 == 0, PD_ERR_SHAPE, "pd_knn_radii: stride f %lld (at least D = %d and a multiple of 4 elements)",
           (long long)a->f_stride, a->D);
  PD_CHECK(((uintptr_t)a->f & 15) == 0, PD_ERR_ARG, "pd_knn_radii: f must be 16-byte aligned");
  PD_CHECK(((uintptr_t)a->rad2 & 7) == 0 && ((uintptr_t)a->workspace & 7) == 0, PD_ERR_ARG, "pd_knn_radii: rad2 / workspace must be 8-byte aligned");
  PD_CHECK(a->N >= 1 && a->N < (1ll << 31), PD_ERR_SHAPE, "pd_knn_radii: N = %lld (1 .. 2^31 - 1 rows)", (long long)a->N);
  PD_CHECK(a->k >= 1 && a->k <= PD_MANIFOLD_MAX_K, PD_ERR_SHAPE, "pd_knn_radii: k = %d (1 .. %d)", a->k, PD_MANIFOLD_MAX_K);
  PD_CHECK(a->k + 1 <= a->N, PD_ERR_SHAPE, "pd_knn_radii: k = %d needs at least k + 1 rows, N = %lld", a->k, (long long)a->N);
  PD_CHECK(a->splits >= 0 && a->splits <= PD_MANIFOLD_MAX_SPLITS, PD_ERR_SHAPE, "pd_knn_radii: splits = %d (0 for the default, or 1 .. %d)", a->splits,
           PD_MANIFOLD_MAX_SPLITS);
  RadLaunch p;
  p.a = *a;
  p.splits = resolve_splits(a->N, a->N, a->splits);
  p.nct = (int)((a->N + TILE - 1) / TILE);
  const int64_t groups = (int64_t)p.nct * p.splits;
  PD_CHECK(groups <= (1ll << 31) - 1, PD_ERR_SHAPE, "pd_knn_radii: grid too large (%lld workgroups, at most 2^31 - 1): fewer splits", (long long)groups);
  const size_t need = radii_workspace(a->N, a->k, a->splits);
  PD_CHECK(a->workspace_bytes >= need, PD_ERR_ARG, "pd_knn_radii: workspace_bytes %zu below the %zu that pd_knn_radii_workspace asks for",
           a->workspace_bytes, need);
  p.norm = (double*)a->workspace;
  p.cand = p.norm + a->N;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(norm_kernel, dim3((unsigned)p.nct), dim3(256), 0, st, a->f, a->f_stride, a->N, a->D, p.norm);
  PD_LAUNCH_CHECK();
  if (a->k + 1 <= 4)
    hipLaunchKernelGGL(radii_tile_kernel<4>, dim3((unsigned)groups), dim3(256), 0, st, p);
  else if (a->k + 1 <= 8)
    hipLaunchKernelGGL(radii_tile_kernel<8>, dim3((unsigned)groups), dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL(radii_tile_kernel<KMAX1>, dim3((unsigned)groups), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(radii_merge_kernel, dim3((unsigned)((a->N + 255) / 256)), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" size_t pd_manifold_query_workspace(int64_t Nq, int64_t Nr, int splits) { return pd::query_workspace(Nq, Nr, splits); }

extern "C" int pd_manifold_query(const pd_manifold_query_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_manifold_query: null args");
  PD_CHECK(a->q != nullptr && a->r != nullptr, PD_ERR_ARG, "pd_manifold_query: null features (q / r)");
  PD_CHECK(a->count != nullptr || a->dmin2 != nullptr, PD_ERR_ARG, "pd_manifold_query: null outputs (count and dmin2 both): nothing to compute");
  PD_CHECK(a->count == nullptr || a->rad2 != nullptr, PD_ERR_ARG, "pd_manifold_query: count needs the radii, and rad2 is null");
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "pd_manifold_query: null workspace (pd_manifold_query_workspace gives its size)");
  PD_CHECK(width_ok(a->D), PD_ERR_SHAPE, "pd_manifold_query: D = %d (a multiple of 64 in 64 .. 4096)", a->D);
  PD_CHECK(a->q_stride >= a->D && a->r_stride >= a->D && a->q_stride % 4 == 0 && a->r_stride % 4 == 0, PD_ERR_SHAPE,
           "pd_manifold_query: stride q %lld / r %lld (at least D = %d and a multiple of 4 elements)", (long long)a->q_stride, (long long)a->r_stride, a->D);
  PD_CHECK(((uintptr_t)a->q & 15) == 0 && ((uintptr_t)a->r & 15) == 0, PD_ERR_ARG, "pd_manifold_query: q / r must be 16-byte aligned");
  PD_CHECK(((uintptr_t)a->rad2 & 7) == 0 && ((uintptr_t)a->dmin2 & 7) == 0 && ((uintptr_t)a->workspace & 7) == 0 && ((uintptr_t)a->count & 3) == 0, PD_ERR_ARG,
           "pd_manifold_query: rad2 / dmin2 / workspace must be 8-byte aligned, count 4-byte aligned");
  PD_CHECK(a->Nq >= 1 && a->Nq < (1ll << 31), PD_ERR_SHAPE, "pd_manifold_query: Nq = %lld (1 .. 2^31 - 1 rows)", (long long)a->Nq);
  PD_CHECK(a->Nr >= 1 && a->Nr < (1ll << 31), PD_ERR_SHAPE, "pd_manifold_query: Nr = %lld (1 .. 2^31 - 1 rows)", (long long)a->Nr);
  PD_CHECK(a->splits >= 0 && a->splits <= PD_MANIFOLD_MAX_SPLITS, PD_ERR_SHAPE, "pd_manifold_query: splits = %d (0 for the default, or 1 .. %d)", a->splits,
           PD_MANIFOLD_MAX_SPLITS);
  QryLaunch p;
  p.a = *a;
  p.splits = resolve_splits(a->Nq, a->Nr, a->splits);
  p.nct = (int)((a->Nr + TILE - 1) / TILE);
  const int64_t rbs = (a->Nq + TILE - 1) / TILE, groups = rbs * p.splits;
  PD_CHECK(groups <= (1ll << 31) - 1, PD_ERR_SHAPE, "pd_manifold_query: grid too large (%lld workgroups, at most 2^31 - 1): fewer splits", (long long)groups);
  const size_t need = query_workspace(a->Nq, a->Nr, a->splits);
  PD_CHECK(a->workspace_bytes >= need, PD_ERR_ARG, "pd_manifold_query: workspace_bytes %zu below the %zu that pd_manifold_query_workspace asks for",
           a->workspace_bytes, need);
  p.nq = (double*)a->workspace;
  p.nr = p.nq + a->Nq;
  p.pmin = p.nr + a->Nr;
  p.pcnt = (int32_t*)(p.pmin + a->Nq * p.splits);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(norm_kernel, dim3((unsigned)rbs), dim3(256), 0, st, a->q, a->q_stride, a->Nq, a->D, p.nq);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(norm_kernel, dim3((unsigned)p.nct), dim3(256), 0, st, a->r, a->r_stride, a->Nr, a->D, p.nr);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(query_tile_kernel, dim3((unsigned)groups), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(query_merge_kernel, dim3((unsigned)((a->Nq + 255) / 256)), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
