// pd_kid_mmd / pd_feature_moments: the statistics of KID and FID in fp64 over fp32 features that stay on the device -- what
// torch-fidelity's metric_kid.py (polynomial-kernel MMD^2 per random subset) and metric_fid.py (mean, np.cov) compute on the host.
// Contract: include/phendiff_hip.h.
//
// Both are Gram products on v_mfma_f64_16x16x4_f64.  Operand maps: lane l = (r = l & 15, g = l >> 4) gives A[row r][k = g] and
// B[k = g][col r], one f64 each; the four results of a lane are C[row g + 4 * reg][col r] (NOT the f32 forms' 4 g + reg).
//
//   pd_kid_mmd          one workgroup (4 waves, 2 x 2, each 32 x 32 = four accumulators) per 64 x 64 tile of one of a subset's three
//                       kernel matrices: XX and YY upper-triangle tiles only (an off-diagonal tile counts twice), XY every tile.  The
//                       gathered rows are staged through LDS as fp32, KC = 32 columns at a time, and widened (exactly) on the way to the
//                       MFMA.  The kernel matrix is never stored: (dot * gamma + coef0)^degree, the selection of valid / off-diagonal
//                       elements and the tile's sum happen in registers; one fp64 partial per tile goes to the workspace and a second
//                       launch folds a subset's partials in tile order.
//   pd_feature_moments  column sums per chunk of 64 rows, folded in chunk order (the mean); then one workgroup per upper-triangle
//                       64 x 64 tile of the covariance, contracting over ALL rows (16 at a time, centred in fp64 before they enter LDS),
//                       which writes its tile and the mirrored one from the same registers (cov is bitwise symmetric).
//
// Determinism: no atomics; every sum runs in one fixed order -- the MFMA's k order, a lane's 16 results, pd_reduce.h's wave and
// workgroup reduction, tiles / chunks by index.  A subset's tiles read only that subset's rows of the index
// tables, so its result does not depend on S or on the other subsets.  Rows at or past m (resp. N) of a ragged tile are not read (zeros are
// staged) and what they would contribute is SELECTED away, never multiplied by zero.
#include <math.h>
#include "pd_reduce.h"

namespace pd {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int TILE = PD_METRIC_STATS_TILE;      // 64 x 64 results per workgroup
constexpr int KC = 32, LDP = KC + 4;            // KID: fp32 columns staged per step; LDS row pitch in floats (144 bytes: 16-byte aligned rows)
constexpr int RK = 16, LDK = TILE + 16;         // moments: rows contracted per step; LDS row pitch in doubles
constexpr int MEAN_ROWS = PD_FEATURE_MOMENTS_CHUNK;

// ---------------------------------------------------------------------------------------------------------------- pd_kid_mmd
struct KidLaunch {
  pd_kid_mmd_args a;
  int nt, tri, tiles;      // tiles per side, nt (nt + 1) / 2, tiles per subset = 2 tri + nt^2: [XX upper | YY upper | XY]
  double* part;            // [S][tiles]
};

__global__ __launch_bounds__(256) void kid_tile_kernel(const KidLaunch p) {
  __shared__ __attribute__((aligned(16))) float sa[TILE * LDP];
  __shared__ __attribute__((aligned(16))) float sb[TILE * LDP];
  __shared__ double red[4];
  const pd_kid_mmd_args& a = p.a;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r16 = lane & 15, g = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const int64_t s = (int64_t)blockIdx.x / p.tiles;
  const int tile = (int)((int64_t)blockIdx.x - s * p.tiles);
  int kind, ti, tj, r = tile;
  if (r < 2 * p.tri) {
    kind = r >= p.tri ? 1 : 0;
    r -= kind * p.tri;
    ti = 0;
    while (r >= p.nt - ti) { r -= p.nt - ti; ++ti; }
    tj = ti + r;
  } else {
    kind = 2;
    r -= 2 * p.tri;
    ti = r / p.nt;
    tj = r - ti * p.nt;
  }
  const float* fa = kind == 1 ? a.f2 : a.f1;
  const float* fb = kind == 0 ? a.f1 : a.f2;
  const int64_t sta = kind == 1 ? a.f2_stride : a.f1_stride, stb = kind == 0 ? a.f1_stride : a.f2_stride;
  const int32_t* ia = (kind == 1 ? a.idx2 : a.idx1) + s * a.idx_stride;
  const int32_t* ib = (kind == 0 ? a.idx1 : a.idx2) + s * a.idx_stride;
  // loader: thread t brings columns 4 (t & 7) .. + 3 of tile rows t >> 3 and 32 + (t >> 3), of either operand
  const int lrow = t >> 3, lc = (t & 7) * 4;
  const float* pa[2];
  const float* pb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int ra = ti * TILE + lrow + 32 * h, rb = tj * TILE + lrow + 32 * h;
    pa[h] = ra < a.m ? fa + (int64_t)ia[ra] * sta + lc : nullptr;
    pb[h] = rb < a.m ? fb + (int64_t)ib[rb] * stb + lc : nullptr;
  }
  f32x4 va[2], vb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      va[h] = pa[h] ? *(const f32x4*)(pa[h] + k0) : (f32x4)(0.f);
      vb[h] = pb[h] ? *(const f32x4*)(pb[h] + k0) : (f32x4)(0.f);
    }
  };
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4)(0.0);
  fetch(0);
  for (int k0 = 0; k0 < a.D; k0 += KC) {
    __syncthreads();      // the previous step's reads are done
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *(f32x4*)&sa[(lrow + 32 * h) * LDP + lc] = va[h];
      *(f32x4*)&sb[(lrow + 32 * h) * LDP + lc] = vb[h];
    }
    __syncthreads();
    if (k0 + KC < a.D) fetch(k0 + KC);
#pragma unroll
    for (int kb = 0; kb < KC / 16; ++kb) {
      // a lane takes 4 consecutive columns and feeds them to 4 MFMAs: MFMA q contracts columns {q, 4 + q, 8 + q, 12 + q} of the block (the
      // same order in both operands)
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
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gi = ti * TILE + wr * 32 + i * 16 + g + 4 * reg, gj = tj * TILE + wc * 32 + j * 16 + r16;
        const double v = acc[i][j][reg] * a.gamma + a.coef0;
        double pw = v;
        for (int d = 1; d < a.degree; ++d) pw *= v;
        const bool keep = gi < a.m && gj < a.m && (kind == 2 || gi != gj);
        sum += keep ? pw : 0.0;
      }
  if (kind != 2 && ti != tj) sum *= 2.0;      // the mirrored tile (exact)
  sum = block_reduce<Sum>(sum, red);
  if (t == 0) p.part[s * p.tiles + tile] = sum;
}

// one workgroup per subset: thread k < 3 folds the partials of matrix k in tile order; thread 0 then forms MMD^2
__global__ __launch_bounds__(64) void kid_fold_kernel(const KidLaunch p) {
  __shared__ double tot[3];
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  if (t < 3) {
    const int b = t * p.tri, e = t < 2 ? b + p.tri : p.tiles;
    const double* in = p.part + s * p.tiles;
    double acc = in[b];
    for (int c = b + 1; c < e; ++c) acc += in[c];
    tot[t] = acc;
    p.a.sums[s * 3 + t] = acc;
  }
  __syncthreads();
  if (t == 0) {
    const double m = (double)p.a.m;
    p.a.mmd[s] = (tot[0] + tot[1]) / (m * (m - 1.0)) - 2.0 * tot[2] / (m * m);
  }
}

// tiles per subset, or 0 where the sizes are refused
int64_t kid_tiles(int64_t S, int64_t m) {
  if (S < 1 || m < 2 || m >= (1ll << 31) || S >= (1ll << 31)) return 0;
  const int64_t nt = (m + TILE - 1) / TILE, tiles = nt * (nt + 1) + nt * nt;
  return tiles > ((1ll << 31) - 1) / S ? 0 : tiles;
}

// ---------------------------------------------------------------------------------------------------------------- pd_feature_moments
struct MomLaunch {
  pd_feature_moments_args a;
  int64_t chunks;      // of MEAN_ROWS rows
  double* part;        // [chunks][D]
};

__global__ __launch_bounds__(64) void colsum_kernel(const MomLaunch p) {
  const int col = blockIdx.y * 64 + threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * MEAN_ROWS, left = p.a.N - n0;
  const int rows = left < MEAN_ROWS ? (int)left : MEAN_ROWS;
  const float* f = p.a.f + n0 * p.a.f_stride + col;
  double acc = 0.0;
  for (int n = 0; n < rows; ++n) acc += (double)f[n * p.a.f_stride];
  p.part[(int64_t)blockIdx.x * p.a.D + col] = acc;
}

__global__ __launch_bounds__(64) void mean_fold_kernel(const MomLaunch p) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  double acc = p.part[col];
  for (int64_t c = 1; c < p.chunks; ++c) acc += p.part[c * p.a.D + col];
  p.a.mean[col] = acc / (double)p.a.N;
}

__global__ __launch_bounds__(256) void cov_tile_kernel(const MomLaunch p) {
  __shared__ __attribute__((aligned(16))) double sa[RK * LDK];
  __shared__ __attribute__((aligned(16))) double sb[RK * LDK];
  const pd_feature_moments_args& a = p.a;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r16 = lane & 15, g = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const int nd = a.D / TILE;
  int ti = 0, r = blockIdx.x;
  while (r >= nd - ti) { r -= nd - ti; ++ti; }
  const int tj = ti + r, i0 = ti * TILE, j0 = tj * TILE;
  // loader: thread t brings columns 4 (t & 15) .. + 3 of row t >> 4 of the step, for both column blocks, centred in fp64
  const int krow = t >> 4, lc = (t & 15) * 4;
  double ma[4], mb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { ma[q] = a.mean[i0 + lc + q]; mb[q] = a.mean[j0 + lc + q]; }
  f32x4 va, vb;
  bool valid = false;
  auto fetch = [&](int64_t n0) {
    const int64_t n = n0 + krow;
    valid = n < a.N;
    const float* row = a.f + n * a.f_stride + lc;
    va = valid ? *(const f32x4*)(row + i0) : (f32x4)(0.f);
    vb = valid ? *(const f32x4*)(row + j0) : (f32x4)(0.f);
  };
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4)(0.0);
  fetch(0);
  for (int64_t n0 = 0; n0 < a.N; n0 += RK) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q += 2) {      // rows at or past N: zero by selection
      *(f64x2*)&sa[krow * LDK + lc + q] = (f64x2){valid ? (double)va[q] - ma[q] : 0.0, valid ? (double)va[q + 1] - ma[q + 1] : 0.0};
      *(f64x2*)&sb[krow * LDK + lc + q] = (f64x2){valid ? (double)vb[q] - mb[q] : 0.0, valid ? (double)vb[q + 1] - mb[q + 1] : 0.0};
    }
    __syncthreads();
    if (n0 + RK < a.N) fetch(n0 + RK);
#pragma unroll
    for (int kq = 0; kq < RK / 4; ++kq) {
      double xa[2], xb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        xa[i] = sa[(kq * 4 + g) * LDK + wr * 32 + i * 16 + r16];
        xb[i] = sb[(kq * 4 + g) * LDK + wc * 32 + i * 16 + r16];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[i], xb[j], acc[i][j], 0, 0, 0);
    }
  }
  const double denom = (double)(a.N - 1);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gi = i0 + wr * 32 + i * 16 + g + 4 * reg, gj = j0 + wc * 32 + j * 16 + r16;
        if (ti != tj || gi <= gj) {      // a diagonal tile writes its upper triangle and mirrors it, like the others
          const double v = acc[i][j][reg] / denom;
          a.cov[(int64_t)gi * a.cov_stride + gj] = v;
          if (gi != gj) a.cov[(int64_t)gj * a.cov_stride + gi] = v;
        }
      }
}

bool width_ok(int D) { return D >= 64 && D <= 4096 && D % 64 == 0; }

int64_t mean_chunks(int64_t N, int D) {
  if (N < 2 || N >= (1ll << 31) || !width_ok(D)) return 0;
  return (N + MEAN_ROWS - 1) / MEAN_ROWS;
}

}  // namespace
}  // namespace pd

extern "C" size_t pd_kid_mmd_workspace(int64_t S, int64_t m) {
  return (size_t)(pd::kid_tiles(S, m) * (S > 0 ? S : 0)) * sizeof(double);
}

extern "C" int pd_kid_mmd(const pd_kid_mmd_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_kid_mmd: null args");
  PD_CHECK(a->f1 != nullptr && a->f2 != nullptr, PD_ERR_ARG, "pd_kid_mmd: null features (f1 / f2)");
  PD_CHECK(a->idx1 != nullptr && a->idx2 != nullptr, PD_ERR_ARG, "pd_kid_mmd: null index table (idx1 / idx2)");
  PD_CHECK(a->sums != nullptr && a->mmd != nullptr, PD_ERR_ARG, "pd_kid_mmd: null output (sums / mmd)");
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "pd_kid_mmd: null workspace (pd_kid_mmd_workspace gives its size)");
  PD_CHECK(width_ok(a->D), PD_ERR_SHAPE, "pd_kid_mmd: D = %d (a multiple of 64 in 64 .. 4096)", a->D);
  PD_CHECK(a->f1_stride >= a->D && a->f2_stride >= a->D && a->f1_stride % 4 == 0 && a->f2_stride % 4 == 0, PD_ERR_SHAPE,
           "pd_kid_mmd: stride f1 %lld / f2 %lld (at least D = %d and a multiple of 4 elements)", (long long)a->f1_stride, (long long)a->f2_stride, a->D);
  PD_CHECK(((uintptr_t)a->f1 & 15) == 0 && ((uintptr_t)a->f2 & 15) == 0, PD_ERR_ARG, "pd_kid_mmd: f1 / f2 must be 16-byte aligned");
  PD_CHECK(a->S >= 1, PD_ERR_SHAPE, "pd_kid_mmd: S = %d subsets (at least 1)", a->S);
  PD_CHECK(a->m >= 2, PD_ERR_SHAPE, "pd_kid_mmd: m = %d (a subset needs at least 2 samples)", a->m);
  PD_CHECK(a->m <= a->N1 && a->m <= a->N2, PD_ERR_SHAPE, "pd_kid_mmd: m = %d exceeds the number of samples (N1 %lld, N2 %lld)", a->m,
           (long long)a->N1, (long long)a->N2);
  PD_CHECK(a->idx_stride >= a->m, PD_ERR_SHAPE, "pd_kid_mmd: idx_stride %lld below m = %d", (long long)a->idx_stride, a->m);
  PD_CHECK(a->degree >= 1 && a->degree <= 8, PD_ERR_ARG, "pd_kid_mmd: degree = %d (1 .. 8)", a->degree);
  PD_CHECK(isfinite(a->gamma), PD_ERR_ARG, "pd_kid_mmd: gamma is not finite");
  PD_CHECK(isfinite(a->coef0), PD_ERR_ARG, "pd_kid_mmd: coef0 is not finite");
  KidLaunch p;
  p.a = *a;
  const int64_t tiles = kid_tiles(a->S, a->m);
  PD_CHECK(tiles > 0, PD_ERR_SHAPE, "pd_kid_mmd: grid too large (S x tiles above 2^31 - 1 workgroups): split the subsets");
  const size_t need = (size_t)(tiles * a->S) * sizeof(double);
  PD_CHECK(a->workspace_bytes >= need, PD_ERR_ARG, "pd_kid_mmd: workspace_bytes %zu below the %zu that pd_kid_mmd_workspace asks for",
           a->workspace_bytes, need);
  p.nt = (a->m + TILE - 1) / TILE;
  p.tri = p.nt * (p.nt + 1) / 2;
  p.tiles = (int)tiles;
  p.part = (double*)a->workspace;
  hipLaunchKernelGGL(kid_tile_kernel, dim3((unsigned)(tiles * a->S)), dim3(256), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(kid_fold_kernel, dim3((unsigned)a->S), dim3(64), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" size_t pd_feature_moments_workspace(int64_t N, int D) {
  return (size_t)(pd::mean_chunks(N, D) * (D > 0 ? D : 0)) * sizeof(double);
}

extern "C" int pd_feature_moments(const pd_feature_moments_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_feature_moments: null args");
  PD_CHECK(a->f != nullptr, PD_ERR_ARG, "pd_feature_moments: null features (f)");
  PD_CHECK(a->mean != nullptr && a->cov != nullptr, PD_ERR_ARG, "pd_feature_moments: null output (mean / cov)");
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "pd_feature_moments: null workspace (pd_feature_moments_workspace gives its size)");
  PD_CHECK(width_ok(a->D), PD_ERR_SHAPE, "pd_feature_moments: D = %d (a multiple of 64 in 64 .. 4096)", a->D);
  PD_CHECK(a->f_stride >= a->D && a->f_stride % 4 == 0, PD_ERR_SHAPE, "pd_feature_moments: stride f %lld (at least D = %d and a multiple of 4 elements)",
           (long long)a->f_stride, a->D);
  PD_CHECK(a->cov_stride >= a->D, PD_ERR_SHAPE, "pd_feature_moments: stride cov %lld below D = %d", (long long)a->cov_stride, a->D);
  PD_CHECK(((uintptr_t)a->f & 15) == 0, PD_ERR_ARG, "pd_feature_moments: f must be 16-byte aligned");
  PD_CHECK(a->N >= 2, PD_ERR_SHAPE, "pd_feature_moments: N = %lld (the unbiased covariance needs at least 2 rows)", (long long)a->N);
  MomLaunch p;
  p.a = *a;
  p.chunks = mean_chunks(a->N, a->D);
  PD_CHECK(p.chunks > 0, PD_ERR_SHAPE, "pd_feature_moments: grid too large (N = %lld, at most 2^31 - 1 rows)", (long long)a->N);
  const size_t need = (size_t)(p.chunks * a->D) * sizeof(double);
  PD_CHECK(a->workspace_bytes >= need, PD_ERR_ARG, "pd_feature_moments: workspace_bytes %zu below the %zu that pd_feature_moments_workspace asks for",
           a->workspace_bytes, need);
  p.part = (double*)a->workspace;
  const int nd = a->D / TILE;
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)p.chunks, (unsigned)nd), dim3(64), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(mean_fold_kernel, dim3((unsigned)nd), dim3(64), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(cov_tile_kernel, dim3((unsigned)(nd * (nd + 1) / 2)), dim3(256), 0, (hipStream_t)stream, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
