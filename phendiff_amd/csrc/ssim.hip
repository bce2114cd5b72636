// pd_ssim: per-(sample, channel, scale) means of the SSIM map and of its contrast-structure factor between two [B][C][H][W] batches that
// stay on the device -- Wang et al.'s SSIM with a separable Gaussian window, valid filtering, and the 2x2-mean pyramid of MS-SSIM.
// Everything after the load is fp64.  Contract: include/phendiff_hip.h; host side phendiff_amd.diagnostics (sample_ssim).
//
// Launches on one stream, no host synchronisation: per scale s >= 1 a reduce launch for x and one for y (level s = 2x2 mean of level s - 1,
// fp64, kept in the workspace), per scale one tiled pass, and one fold launch for all (plane, scale) pairs at the end.
//
// The tiled pass: a workgroup of 256 threads owns TH x TW = 16 x 32 positions of the valid map of one (sample, channel) plane.  It stages
// the (TH + win - 1) x (TW + win - 1) rectangle of x and of y in LDS as fp64, filters the rows into five maps (x, y, x^2, y^2, xy) of
// (TH + win - 1) x TW in LDS, filters the columns of those, evaluates ssim / cs and reduces them to one pair per workgroup.
// LDS: 8 * (2 (15 + win)(31 + win) + 5 (15 + win) 32) bytes = 50,752 at win 11 (three workgroups per CU), 110,592 at win 33 (one).
// Lane = column in every phase, so the 8-byte LDS accesses of a 32-lane group are consecutive: conflict-free.
//
// Over-reads: a position outside the plane is never loaded; its LDS slot gets 0.0 by selection, and a map position that would need it
// lies outside the valid map and is left out of the sums by selection, never multiplied by zero.
//
// Determinism: element loads only, so nothing depends on alignment; which thread takes which position depends on the position within the
// plane only; the sums over a tile's positions and over a plane's tiles run in the one fixed order of pd_reduce.h.  No floating-point atomics.
#include <math.h>
#include <stddef.h>
#include "pd_reduce.h"

namespace pd {
namespace {

constexpr int TH = 16, TW = 32, NT = 256, MAXW = PD_SSIM_MAX_WIN, MAXL = PD_SSIM_MAX_LEVELS;
static_assert(NT == 256, "pd_reduce.h's block_reduce and run_fold are written for workgroups of 256 threads (four waves)");
static_assert(offsetof(pd_ssim_args, w32) - offsetof(pd_ssim_args, w0) == (MAXW - 1) * sizeof(double), "the taps w0..w32 are one run of doubles");

__device__ __forceinline__ double widen(float v) { return (double)v; }
__device__ __forceinline__ double widen(bf16_t v) { return (double)bf2f(v); }
__device__ __forceinline__ double widen(half_t v) { return (double)h2f(v); }
__device__ __forceinline__ double widen(double v) { return v; }

struct Pass {
  const void* x; const void* y;      // level s of both: [planes][H][W] (y: [C][H][W] when shared)
  double* part;                      // [planes][tiles][2]
  int C, H, W, win, tiles_x, tiles_y, y_shared;
  double c1, c2;
  double window[MAXW];
};

struct Fold {
  const double* part[MAXL];
  int64_t tiles[MAXL];
  double npos[MAXL];
  int levels;
  double* out;                       // [planes][levels][2]
};

template <typename T> __global__ __launch_bounds__(NT) void ssim_pass_kernel(const Pass p) {
  extern __shared__ double lds[];
  __shared__ double red[NT / 64][2];
  const int win = p.win, halo = win - 1, IR = TH + halo, IC = TW + halo, t = threadIdx.x;
  double* X = lds;                   // [IR][IC]
  double* Y = X + IR * IC;           // [IR][IC]
  double* M = Y + IR * IC;           // [5][IR][TW]: rows filtered
  const int64_t tiles = (int64_t)p.tiles_x * p.tiles_y, blk = blockIdx.x, plane = blk / tiles, tile = blk - plane * tiles;
  const int ty0 = (int)(tile / p.tiles_x) * TH, tx0 = (int)(tile % p.tiles_x) * TW;
  const int64_t hw = (int64_t)p.H * p.W;
  const T* x = (const T*)p.x + plane * hw;
  const T* y = (const T*)p.y + (p.y_shared ? plane % p.C : plane) * hw;

  for (int i = t; i < IR * IC; i += NT) {
    const int r = i / IC, c = i - r * IC, gy = ty0 + r, gx = tx0 + c;
    double xv = 0.0, yv = 0.0;
    if (gy < p.H && gx < p.W) {
      const int64_t off = (int64_t)gy * p.W + gx;
      xv = widen(x[off]);
      yv = widen(y[off]);
    }
    X[i] = xv;
    Y[i] = yv;
  }
  __syncthreads();

  const int plane_m = IR * TW;
  for (int i = t; i < plane_m; i += NT) {
    const int r = i / TW, c = i - r * TW;
    const double* xr = X + r * IC + c;
    const double* yr = Y + r * IC + c;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int k = 0; k < win; ++k) {
      const double xv = xr[k], yv = yr[k], gx = p.window[k] * xv, gy = p.window[k] * yv;
      sx += gx;
      sy += gy;
      sxx = fma(gx, xv, sxx);
      syy = fma(gy, yv, syy);
      sxy = fma(gx, yv, sxy);
    }
    M[i] = sx;
    M[plane_m + i] = sy;
    M[2 * plane_m + i] = sxx;
    M[3 * plane_m + i] = syy;
    M[4 * plane_m + i] = sxy;
  }
  __syncthreads();

  const int Hv = p.H - halo, Wv = p.W - halo;
  double acc[2] = {0.0, 0.0};
  for (int i = t; i < TH * TW; i += NT) {
    const int r = i / TW, c = i - r * TW;
    if (ty0 + r < Hv && tx0 + c < Wv) {      // (uniform over each half wave: a row of the tile)
      const double* m = M + r * TW + c;
      double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
      for (int k = 0; k < win; ++k) {
        const double g = p.window[k];
        const double* mk = m + k * TW;
        mx = fma(g, mk[0], mx);
        my = fma(g, mk[plane_m], my);
        exx = fma(g, mk[2 * plane_m], exx);
        eyy = fma(g, mk[3 * plane_m], eyy);
        exy = fma(g, mk[4 * plane_m], exy);
      }
      const double vx = exx - mx * mx, vy = eyy - my * my, vxy = exy - mx * my;
      const double cs = (2.0 * vxy + p.c2) / (vx + vy + p.c2);
      acc[0] += cs * ((2.0 * mx * my + p.c1) / (mx * mx + my * my + p.c1));
      acc[1] += cs;
    }
  }
  block_reduce(Ops<Sum, Sum>(), acc, red);
  if (t == 0) { p.part[blk * 2] = acc[0]; p.part[blk * 2 + 1] = acc[1]; }
}

// level s from level s - 1: one thread per output element, rows and columns past the last whole pair are dropped
template <typename T> __global__ __launch_bounds__(NT) void ssim_reduce_kernel(const T* src, double* dst, int64_t total, int Hs, int Ws, int Hd, int Wd) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / Wd, plane = row / Hd;
  const int px = (int)(i - row * Wd), py = (int)(row - plane * Hd);
  const T* s = src + (plane * Hs + 2 * py) * (int64_t)Ws + 2 * px;
  dst[i] = ((widen(s[0]) + widen(s[1])) + (widen(s[Ws]) + widen(s[Ws + 1]))) * 0.25;
}

// one workgroup per (plane, scale) folds the plane's tiles
__global__ __launch_bounds__(NT) void ssim_fold_kernel(const Fold p) {
  __shared__ double red[NT][2];
  const int64_t blk = blockIdx.x, plane = blk / p.levels;
  const int s = (int)(blk - plane * p.levels);
  double r[2];
  run_fold(Ops<Sum, Sum>(), p.part[s] + plane * p.tiles[s] * 2, p.tiles[s], red, r);
  if (threadIdx.x == 0) { p.out[blk * 2] = r[0] / p.npos[s]; p.out[blk * 2 + 1] = r[1] / p.npos[s]; }
}

// where everything lives, from the sizes alone (the query knows neither win nor whether y is shared: the partials are sized for the smallest
// window, 3, and the pyramid of y for one y per sample)
struct Plan {
  int64_t planes, total;             // total: doubles of workspace
  int Hs[MAXL], Ws[MAXL];
  int64_t part_off[MAXL], pyr_off[MAXL], pyr_y;      // doubles; level s of y at pyr_y + pyr_off[s]
};

int64_t tiles_of(int Hs, int Ws, int win, int* tx, int* ty) {
  *tx = (Ws - win + 1 + TW - 1) / TW;
  *ty = (Hs - win + 1 + TH - 1) / TH;
  return (int64_t)*tx * *ty;
}

// false where the sizes are refused
bool make_plan(int64_t B, int C, int H, int W, int levels, Plan& pl) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || levels < 1 || levels > MAXL) return false;
  if (((H < W ? H : W) >> (levels - 1)) < 3) return false;
  const int64_t hw = (int64_t)H * W, lim = 1ll << 40;      // elements per batch: keeps every offset and the workspace's size in int64
  if (hw > lim || C > lim / hw || B > lim / (hw * C)) return false;
  pl.planes = B * C;
  int t0x, t0y;
  const int64_t max_grid = (1ll << 31) - 1;
  if (pl.planes > max_grid / tiles_of(H, W, 3, &t0x, &t0y) || pl.planes > max_grid / MAXL) return false;
  int64_t off = 0;
  for (int s = 0; s < levels; ++s) {
    int tx, ty;
    pl.Hs[s] = H >> s;
    pl.Ws[s] = W >> s;
    pl.part_off[s] = off;
    off += pl.planes * tiles_of(pl.Hs[s], pl.Ws[s], 3, &tx, &ty) * 2;
  }
  const int64_t pyr0 = off;
  for (int s = 1; s < levels; ++s) {
    pl.pyr_off[s] = off;
    off += pl.planes * pl.Hs[s] * pl.Ws[s];
  }
  pl.pyr_off[0] = pyr0;
  pl.pyr_y = off - pyr0;
  pl.total = off + pl.pyr_y;
  return true;
}

template <typename T> int launch_pass(const Pass& p, int64_t planes, hipStream_t st) {
  static LdsAttr attr;
  const int IR = TH + p.win - 1, IC = TW + p.win - 1;
  const size_t lds = (size_t)(2 * IR * IC + 5 * IR * TW) * sizeof(double);
  PD_CHECK(ensure_lds(attr, ssim_pass_kernel<T>, (int)((2 * (TH + MAXW - 1) * (TW + MAXW - 1) + 5 * (TH + MAXW - 1) * TW) * sizeof(double))),
           PD_ERR_LAUNCH, "pd_ssim: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL(ssim_pass_kernel<T>, dim3((unsigned)(planes * p.tiles_x * p.tiles_y)), dim3(NT), lds, st, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

template <typename T> int launch_reduce(const T* src, double* dst, int64_t planes, int Hs, int Ws, hipStream_t st) {
  const int Hd = Hs >> 1, Wd = Ws >> 1;
  const int64_t total = planes * Hd * Wd;
  hipLaunchKernelGGL(ssim_reduce_kernel<T>, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, src, dst, total, Hs, Ws, Hd, Wd);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

template <typename T> int launch_all(const pd_ssim_args& a, const Plan& pl, hipStream_t st) {
  double* ws = (double*)a.workspace;
  const bool shared = a.y_sample_stride == 0;
  const int64_t yplanes = shared ? a.C : pl.planes;
  Pass p;
  p.C = a.C; p.win = a.win; p.y_shared = shared ? 1 : 0; p.c1 = a.c1; p.c2 = a.c2;
  for (int k = 0; k < MAXW; ++k) p.window[k] = k < a.win ? (&a.w0)[k] : 0.0;
  Fold f;
  f.levels = a.levels; f.out = a.out;
  for (int s = 0; s < a.levels; ++s) {
    const double* px = ws + pl.pyr_off[s];
    const double* py = px + pl.pyr_y;
    if (s == 1) {
      int rc = launch_reduce<T>((const T*)a.x, (double*)px, pl.planes, pl.Hs[0], pl.Ws[0], st);
      if (rc == PD_OK) rc = launch_reduce<T>((const T*)a.y, (double*)py, yplanes, pl.Hs[0], pl.Ws[0], st);
      if (rc != PD_OK) return rc;
    } else if (s > 1) {
      int rc = launch_reduce<double>(ws + pl.pyr_off[s - 1], (double*)px, pl.planes, pl.Hs[s - 1], pl.Ws[s - 1], st);
      if (rc == PD_OK) rc = launch_reduce<double>(ws + pl.pyr_off[s - 1] + pl.pyr_y, (double*)py, yplanes, pl.Hs[s - 1], pl.Ws[s - 1], st);
      if (rc != PD_OK) return rc;
    }
    p.H = pl.Hs[s]; p.W = pl.Ws[s];
    p.part = ws + pl.part_off[s];
    f.tiles[s] = tiles_of(p.H, p.W, a.win, &p.tiles_x, &p.tiles_y);
    f.part[s] = p.part;
    f.npos[s] = (double)(p.H - a.win + 1) * (double)(p.W - a.win + 1);
    p.x = s ? (const void*)px : a.x;
    p.y = s ? (const void*)py : a.y;
    const int rc = s ? launch_pass<double>(p, pl.planes, st) : launch_pass<T>(p, pl.planes, st);
    if (rc != PD_OK) return rc;
  }
  for (int s = a.levels; s < MAXL; ++s) { f.part[s] = nullptr; f.tiles[s] = 0; f.npos[s] = 1.0; }
  hipLaunchKernelGGL(ssim_fold_kernel, dim3((unsigned)(pl.planes * a.levels)), dim3(NT), 0, st, f);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // namespace
}  // namespace pd

extern "C" size_t pd_ssim_workspace(int64_t B, int C, int H, int W, int levels) {
  pd::Plan pl;
  return pd::make_plan(B, C, H, W, levels, pl) ? (size_t)pl.total * sizeof(double) : 0;
}

extern "C" int pd_ssim(const pd_ssim_args* a, void* stream) {
  using namespace pd;
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_ssim: null args");
  PD_CHECK(a->x != nullptr && a->y != nullptr, PD_ERR_ARG, "pd_ssim: null %s", a->x ? "y" : "x");
  PD_CHECK(a->out != nullptr, PD_ERR_ARG, "pd_ssim: null out");
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "pd_ssim: null workspace (pd_ssim_workspace gives its size)");
  PD_CHECK(a->dtype == PD_F32 || a->dtype == PD_BF16 || a->dtype == PD_F16, PD_ERR_ARG, "pd_ssim: dtype %d (PD_F32 / PD_BF16 / PD_F16)", a->dtype);
  PD_CHECK(__builtin_isfinite(a->c1) && __builtin_isfinite(a->c2) && a->c1 > 0.0 && a->c2 > 0.0, PD_ERR_ARG, "pd_ssim: c1 = %g, c2 = %g (finite and positive)", a->c1, a->c2);
  PD_CHECK(a->B > 0 && a->C > 0 && a->H > 0 && a->W > 0, PD_ERR_SHAPE, "pd_ssim: shape [%lld][%d][%d][%d]: B, C, H, W must be positive",
           (long long)a->B, a->C, a->H, a->W);
  PD_CHECK(a->win >= 3 && a->win <= MAXW && (a->win & 1), PD_ERR_SHAPE, "pd_ssim: window of %d taps (odd, 3 .. %d)", a->win, MAXW);
  for (int k = 0; k < a->win; ++k) PD_CHECK(__builtin_isfinite((&a->w0)[k]), PD_ERR_ARG, "pd_ssim: window tap %d is not finite", k);
  PD_CHECK(a->levels >= 1 && a->levels <= MAXL, PD_ERR_SHAPE, "pd_ssim: levels = %d (1 .. %d)", a->levels, MAXL);
  const int least = (a->H < a->W ? a->H : a->W) >> (a->levels - 1);
  PD_CHECK(least >= a->win, PD_ERR_SHAPE, "pd_ssim: shape %d x %d: min(H, W) >> (levels - 1) = %d is below the window's %d taps (levels = %d)",
           a->H, a->W, least, a->win, a->levels);
  Plan pl;
  PD_CHECK(make_plan(a->B, a->C, a->H, a->W, a->levels, pl), PD_ERR_SHAPE, "pd_ssim: shape [%lld][%d][%d][%d] is past the index range (2^40 elements, 2^31 - 1 workgroups): split the batch",
           (long long)a->B, a->C, a->H, a->W);
  PD_CHECK(a->y_sample_stride == 0 || a->y_sample_stride == (int64_t)a->C * a->H * a->W, PD_ERR_SHAPE,
           "pd_ssim: y_sample_stride %lld (C * H * W = %lld for one y per sample, 0 to share one)", (long long)a->y_sample_stride,
           (long long)((int64_t)a->C * a->H * a->W));
  const size_t need = (size_t)pl.total * sizeof(double);
  PD_CHECK(a->workspace_bytes >= need, PD_ERR_ARG, "pd_ssim: workspace_bytes %zu below the %zu that pd_ssim_workspace asks for", a->workspace_bytes, need);
  switch (a->dtype) {
    case PD_F32: return launch_all<float>(*a, pl, (hipStream_t)stream);
    case PD_BF16: return launch_all<bf16_t>(*a, pl, (hipStream_t)stream);
    default: return launch_all<half_t>(*a, pl, (hipStream_t)stream);
  }
}
