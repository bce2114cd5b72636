// Tiled trajectories (phendiff_amd/tiling.py): the working sample is a canvas (B, C, Hc, Wc), the UNet sees overlapping tiles of the size it
// was trained at, and their outputs are blended back into one canvas-sized model output.  All tensors fp32 NCHW, what a launch plan reads
// and writes.
//   pd_tile_gather   tiles [first, first + count) of the canvas -> a dense tile batch (count, C, th, tw); a copy, bit for bit
//   pd_tile_blend    out(b, c, y, x) = sum over the tiles (ky, kx) of image b that cover (y, x), ky ascending then kx ascending, of
//                    (wy[ky][y - y0] * wx[kx][x - x0]) * tile(b, ky, kx)(c, y - y0, x - x0)
//                    the weight product, each term and each addition rounded to fp32 on their own (contraction off); the first term is
//                    taken as it is (no zero in front), so a position covered once with weight 1 is a copy
// The grid is a tensor product of two axes.  Per axis: tile k starts at min(k * stride, L - t), so the last tile is flush with the edge; any
// number of tiles may cover a position (L = 72, t = 32, stride 16: origins 0, 16, 32, 40, rows 40..47 three times).
//
// Both kernels are in gather form: one thread per 4 consecutive positions of a row (or per position) of what is WRITTEN reads what it
// needs, so every output element is written exactly once by one thread -- no atomics, no cleared memory, a function of the inputs alone.
// Memory-bound streams: consecutive lanes take consecutive positions of a row, 16 bytes per lane where every tile origin along x, Wc and tw
// are multiples of 4 and the pointers are 16-byte aligned (then a group of 4 lies wholly inside or outside every tile, at a 16-byte
// aligned place of tile, weight row and canvas); 4 bytes per lane otherwise (a flush origin such as x0 = 3).  No LDS, 11 to 40 VGPRs, no
// scratch: occupancy is at the cap of 8 waves per SIMD; the loads of the covering tiles of a position do not depend on each other.
#include "pd_common.h"

namespace pd {

constexpr int TILE_THREADS = 256;

struct TileGeom { int B, C, Hc, Wc, th, tw, nty, ntx, sy, sx; };

__device__ __forceinline__ int tile_origin(int k, int stride, int last) { const int o = k * stride; return o < last ? o : last; }
// the first tile of an axis that can cover position p: tiles with k * stride + t <= p end before it (their origin is at most k * stride)
__device__ __forceinline__ int tile_first_covering(int p, int t, int stride) { return p >= t ? (p - t) / stride + 1 : 0; }

// grid: groups of E positions of the tile batch [count][C][th][tw]
template <bool VEC>
__global__ __launch_bounds__(TILE_THREADS) void tile_gather_kernel(const TileGeom g, const int first, const unsigned groups,
                                                                   const float* __restrict__ canvas, float* __restrict__ tiles) {
  constexpr int E = VEC ? 4 : 1;
  const unsigned i = blockIdx.x * (unsigned)TILE_THREADS + threadIdx.x;
  if (i >= groups) return;
  const unsigned gw = (unsigned)g.tw / E;
  unsigned r = i;
  const unsigned xg = r % gw; r /= gw;
  const unsigned y = r % (unsigned)g.th; r /= (unsigned)g.th;
  const unsigned c = r % (unsigned)g.C; r /= (unsigned)g.C;
  const unsigned t = (unsigned)first + r;                               // tile order: b, then ky, then kx
  const unsigned kx = t % (unsigned)g.ntx, ky = (t / (unsigned)g.ntx) % (unsigned)g.nty, b = t / (unsigned)(g.ntx * g.nty);
  const int y0 = tile_origin((int)ky, g.sy, g.Hc - g.th), x0 = tile_origin((int)kx, g.sx, g.Wc - g.tw);
  const size_t src = (((size_t)b * g.C + c) * g.Hc + (y0 + y)) * g.Wc + x0 + xg * E;
  if (VEC) *(f32x4*)(tiles + (size_t)i * 4) = *(const f32x4*)(canvas + src);
  else tiles[i] = canvas[src];
}

// grid: groups of E positions of the canvas [B][C][Hc][Wc]
template <bool VEC>
__global__ __launch_bounds__(TILE_THREADS) void tile_blend_kernel(const TileGeom g, const unsigned groups, const float* __restrict__ tiles,
                                                                  const float* __restrict__ wy, const float* __restrict__ wx,
                                                                  float* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int E = VEC ? 4 : 1;
  const unsigned i = blockIdx.x * (unsigned)TILE_THREADS + threadIdx.x;
  if (i >= groups) return;
  const unsigned gw = (unsigned)g.Wc / E;
  unsigned r = i;
  const int x = (int)(r % gw) * E; r /= gw;
  const int y = (int)(r % (unsigned)g.Hc); r /= (unsigned)g.Hc;
  const unsigned c = r % (unsigned)g.C, b = r / (unsigned)g.C;
  float acc[E];
  bool any = false;
  for (int ky = tile_first_covering(y, g.th, g.sy); ky < g.nty; ++ky) {
    const int y0 = tile_origin(ky, g.sy, g.Hc - g.th);
    if (y0 > y) break;                                                  // (origins do not decrease with k)
    if (y - y0 >= g.th) continue;
    const float vy = wy[ky * g.th + (y - y0)];
    for (int kx = tile_first_covering(x, g.tw, g.sx); kx < g.ntx; ++kx) {
      const int x0 = tile_origin(kx, g.sx, g.Wc - g.tw);
      if (x0 > x) break;
      if (x - x0 >= g.tw) continue;
      const size_t t = ((size_t)b * g.nty + ky) * g.ntx + kx;
      const size_t src = ((t * g.C + c) * g.th + (y - y0)) * g.tw + (x - x0);
      float m[E], vx[E];
      if (VEC) {
        const f32x4 mv = *(const f32x4*)(tiles + src), wv = *(const f32x4*)(wx + kx * g.tw + (x - x0));
#pragma unroll
        for (int e = 0; e < E; ++e) { m[e] = mv[e]; vx[e] = wv[e]; }
      } else {
        m[0] = tiles[src]; vx[0] = wx[kx * g.tw + (x - x0)];
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float w = vy * vx[e];
        const float term = w * m[e];
        acc[e] = any ? acc[e] + term : term;
      }
      any = true;
    }
  }
  // (the entry point refuses a grid that leaves a position uncovered, so `any` holds; a position is written in any case)
  if (!any) {
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
  }
  if (VEC) *(f32x4*)(out + (size_t)i * 4) = (f32x4){acc[0], acc[E > 1 ? 1 : 0], acc[E > 2 ? 2 : 0], acc[E > 3 ? 3 : 0]};
  else out[i] = acc[0];
}

static int64_t axis_tiles(int64_t L, int64_t t, int64_t s) { return (L - t + s - 1) / s + 1; }

// what both entry points refuse about the grid; T <- B * nty * ntx
static int tile_geom_validate(const TileGeom& g, int64_t* T, const char* who) {
  PD_CHECK(g.B >= 1 && g.C >= 1 && g.Hc >= 1 && g.Wc >= 1, PD_ERR_SHAPE, "%s: canvas (B, C, Hc, Wc) = (%d, %d, %d, %d) (all must be >= 1)", who,
           g.B, g.C, g.Hc, g.Wc);
  PD_CHECK(g.th >= 1 && g.tw >= 1, PD_ERR_SHAPE, "%s: tile %d x %d (both must be >= 1)", who, g.th, g.tw);
  PD_CHECK(g.th <= g.Hc && g.tw <= g.Wc, PD_ERR_SHAPE, "%s: tile %d x %d is larger than the canvas %d x %d", who, g.th, g.tw, g.Hc, g.Wc);
  PD_CHECK(g.sy >= 1 && g.sy <= g.th && g.sx >= 1 && g.sx <= g.tw, PD_ERR_SHAPE,
           "%s: stride (%d, %d) for a %d x %d tile (1 <= stride <= tile: the overlap is tile - stride)", who, g.sy, g.sx, g.th, g.tw);
  PD_CHECK(g.nty == axis_tiles(g.Hc, g.th, g.sy) && g.ntx == axis_tiles(g.Wc, g.tw, g.sx), PD_ERR_SHAPE,
           "%s: tile counts (%d, %d), the grid has ceil((L - t) / stride) + 1 = (%lld, %lld)", who, g.nty, g.ntx,
           (long long)axis_tiles(g.Hc, g.th, g.sy), (long long)axis_tiles(g.Wc, g.tw, g.sx));
  *T = (int64_t)g.B * g.nty * g.ntx;
  PD_CHECK((int64_t)g.B * g.C * g.Hc * g.Wc < (1ll << 31), PD_ERR_SHAPE, "%s: a canvas of %lld elements overflows 32-bit offsets (must be below 2^31)",
           who, (long long)((int64_t)g.B * g.C * g.Hc * g.Wc));
  return PD_OK;
}

static int tile_batch_validate(const TileGeom& g, int64_t tiles, const char* who) {
  const int64_t per_tile = (int64_t)g.C * g.th * g.tw;
  PD_CHECK(tiles < (1ll << 31) && tiles * per_tile < (1ll << 31), PD_ERR_SHAPE,
           "%s: a tile batch of %lld x %lld elements overflows 32-bit offsets (must be below 2^31)", who, (long long)tiles, (long long)per_tile);
  return PD_OK;
}

// 16 bytes per lane: every origin along x, the canvas width and the tile width are multiples of 4 (the flush origin is Wc - tw)
static bool tile_vec_ok(const TileGeom& g, const void* p0, const void* p1, const void* p2) {
  return g.Wc % 4 == 0 && g.tw % 4 == 0 && (g.ntx == 1 || g.sx % 4 == 0) && (uintptr_t)p0 % 16 == 0 && (uintptr_t)p1 % 16 == 0 &&
         (uintptr_t)p2 % 16 == 0;
}

}  // namespace pd

using namespace pd;

extern "C" int pd_tile_gather(const pd_tile_gather_args* a, void* stream) {
  const char* const name = "pd_tile_gather";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", name);
  PD_CHECK(a->canvas && a->tiles, PD_ERR_ARG, "%s: null pointer (canvas, tiles)", name);
  const TileGeom g = {a->B, a->C, a->Hc, a->Wc, a->th, a->tw, a->nty, a->ntx, a->sy, a->sx};
  int64_t T = 0;
  int rc = tile_geom_validate(g, &T, name);
  if (rc != PD_OK) return rc;
  PD_CHECK(a->first >= 0 && a->count >= 1 && (int64_t)a->first + a->count <= T, PD_ERR_SHAPE,
           "%s: tiles [%d, %d + %d) of %lld (first >= 0, count >= 1, first + count <= B * nty * ntx)", name, a->first, a->first, a->count,
           (long long)T);
  rc = tile_batch_validate(g, a->count, name);
  if (rc != PD_OK) return rc;
  PD_CHECK((uintptr_t)a->canvas % 4 == 0 && (uintptr_t)a->tiles % 4 == 0, PD_ERR_ARG, "%s: canvas / tiles must be 4-byte aligned", name);
  const bool vec = tile_vec_ok(g, a->canvas, a->tiles, nullptr);
  const int64_t groups = (int64_t)a->count * g.C * g.th * g.tw / (vec ? 4 : 1);
  const dim3 grid((unsigned)((groups + TILE_THREADS - 1) / TILE_THREADS));
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(tile_gather_kernel<true>, grid, dim3(TILE_THREADS), 0, st, g, a->first, (unsigned)groups, a->canvas, a->tiles);
  else hipLaunchKernelGGL(tile_gather_kernel<false>, grid, dim3(TILE_THREADS), 0, st, g, a->first, (unsigned)groups, a->canvas, a->tiles);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_tile_blend(const pd_tile_blend_args* a, void* stream) {
  const char* const name = "pd_tile_blend";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", name);
  PD_CHECK(a->tiles && a->wy && a->wx && a->out, PD_ERR_ARG, "%s: null pointer (tiles, wy, wx, out)", name);
  const TileGeom g = {a->B, a->C, a->Hc, a->Wc, a->th, a->tw, a->nty, a->ntx, a->sy, a->sx};
  int64_t T = 0;
  int rc = tile_geom_validate(g, &T, name);
  if (rc != PD_OK) return rc;
  rc = tile_batch_validate(g, T, name);
  if (rc != PD_OK) return rc;
  PD_CHECK((uintptr_t)a->tiles % 4 == 0 && (uintptr_t)a->wy % 4 == 0 && (uintptr_t)a->wx % 4 == 0 && (uintptr_t)a->out % 4 == 0, PD_ERR_ARG,
           "%s: tiles / wy / wx / out must be 4-byte aligned", name);
  const bool vec = tile_vec_ok(g, a->tiles, a->wx, a->out);
  const int64_t groups = (int64_t)g.B * g.C * g.Hc * g.Wc / (vec ? 4 : 1);
  const dim3 grid((unsigned)((groups + TILE_THREADS - 1) / TILE_THREADS));
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(tile_blend_kernel<true>, grid, dim3(TILE_THREADS), 0, st, g, (unsigned)groups, a->tiles, a->wy, a->wx, a->out);
  else hipLaunchKernelGGL(tile_blend_kernel<false>, grid, dim3(TILE_THREADS), 0, st, g, (unsigned)groups, a->tiles, a->wy, a->wx, a->out);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
