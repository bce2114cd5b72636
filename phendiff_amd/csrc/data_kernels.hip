// Image preprocessing: decoded uint8 images -> the engine's float32 NCHW input (and the uint8 "raw" twin of the metric reference sets).
//   pd_image_preprocess   Resize(BILINEAR) -> ToTensor -> Normalize [-> RandomHorizontalFlip -> RandomVerticalFlip] of
//                         src/utils_dataset.py:104-127 and src/utils_Img2Img.py:197-206, which the reference runs per image in PIL on the host.
//   pd_image_preprocess_bands   the same transform for stacks of 1..32 independent bands (C in, C out); both kernels call ip_resample_tile.
// The resize is Pillow's 8-bit bilinear resample restated in the same integer arithmetic (ImagingResample: separable, antialiasing support
// max(scale, 1), 22-bit fixed-point coefficients, accumulator 1 << 21, >> 22, clamp; horizontal pass first INTO uint8, then the vertical
// pass; an axis whose size does not change is skipped, not run through an identity table), so the output is held to bit equality.  The
// host builds the coefficient tables in float64 (phendiff_amd/data.py resample_tables) and passes them in.
//
// Kernel shape.  One workgroup (256 threads) owns one 8 x 32 output tile of one image:
//   1. its coefficients and (clamped, tile-relative) bounds go to LDS;
//   2. the source rows the tile's 8 output rows need are streamed global -> LDS in chunks of R rows, only the columns the tile's 32
//      output columns need, as whole dwords wherever a dword lies inside the segment (single bytes at its two ragged ends, so nothing
//      outside the segment is ever read), and each chunk is run through the horizontal pass into the uint8 intermediate
//      [source rows of the tile][32 x Cin], which stays in LDS;
//   3. the vertical pass runs over the intermediate into an 8 x 32 x Cin uint8 tile;
//   4. the tile is written as uint8 NHWC bytes and / or converted ((float)v / 255 - mean) / std and written NCHW at the mirrored position.
// Tile size.  At the training shape (1024 x 1280 -> 128 x 128: scale 8 x 10, 17 x 21 taps) a tile spans 74 source rows x 332 source
// columns: the intermediate is 7 KiB, the tables 3 KiB, a staged row 1 KiB.  R is chosen so that the whole workgroup stays within 40 KiB of
// the CU's 160 KiB of LDS -- four workgroups = 16 waves per CU, enough to hide the source loads behind the other workgroups' passes -- and
// 64 KiB (no opt-in attribute) is the hard ceiling, reached only near the 32 x down-scale limit on both axes.  Horizontally adjacent tiles
// share 2 x support columns (332 read for 320 owned: 4 %), vertically adjacent ones 2 x support rows (74 for 64: 14 %, re-read from L2),
// so every source byte comes from HBM about once.  A wider tile would cut the shared columns further but the 128-wide training output
// gives only 4 tiles per row as it is; a taller one doubles the intermediate at the down-scale limit (290 rows x 96 B at 8 rows).
// Every table value is clamped before it indexes anything: a malformed table gives wrong pixels, never an access outside the operands.
#include "pd_common.h"

namespace pd {

constexpr int IP_TOH = 8, IP_TOW = 32, IP_THREADS = 256;
constexpr int IP_MAX_KSIZE = 65;                 // 2 * 32 + 1: the 32 x down-scale limit
constexpr int IP_LDS_TARGET = 40 * 1024, IP_LDS_MAX = 64 * 1024;

// what the host derives from the shapes (the tables are device memory: the host never reads them)
struct ip_plan {
  int span_x, span_y;     // upper bounds of the source columns / rows one tile needs
  int lrow;               // bytes of one staged source row in LDS (multiple of 4; 3 bytes of slack for the global address' low bits)
  int irow;               // bytes of one intermediate / output-tile row (multiple of 4)
  int chunk_rows;         // R
  int off_cy, off_bnd, off_inter, off_stage, off_out, lds_bytes;   // LDS layout (coef_x at 0)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Pillow's clip8 of the 22-bit fixed-point accumulator (accumulated with wrap-around: defined for any table)
__device__ __forceinline__ unsigned char clip8(uint32_t acc) {
  const int v = (int)acc >> 22;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The resample of one 8 x 32 output tile of image `n`, shared by the two entry points so that they cannot drift: channels
// [cbase, cbase + ci) of every source pixel, each one an independent 8-bit band, through the horizontal and then the vertical pass.
// `A` is either args struct (the geometry and table fields carry the same names).  CI > 0: the channel count at compile time (the
// RGB / grey entry), CI == 0: `ci_rt` channels (the band entry).  Returns the tile in LDS, [th][P.irow] bytes with byte ox * ci + c of
// a row = channel cbase + c of output column ox0 + ox; ends with a barrier.
template <int CI, typename A>
__device__ __forceinline__ const unsigned char* ip_resample_tile(const A& a, const ip_plan& P, unsigned char* smem, int n, int cbase, int ci_rt,
                                                                 int ox0, int oy0, int tw, int th) {
  const int ci = CI ? CI : ci_rt;
  int* const cx = (int*)smem;
  int* const cy = (int*)(smem + P.off_cy);
  int* const bx = (int*)(smem + P.off_bnd);          // [IP_TOW][2]: first source column relative to the tile's x0, count
  int* const by = bx + 2 * IP_TOW;                   // [IP_TOH][2]
  unsigned char* const inter = smem + P.off_inter;
  unsigned char* const stage = smem + P.off_stage;
  unsigned char* const outt = smem + P.off_out;

  const int tid = threadIdx.x;
  const bool rx = a.W != a.OW, ry = a.H != a.OH;
  const int ps = a.pixel_stride;

  // the tile's source window [x0, x1) x [y0, y1): the bounds are monotone in the output index, so the first output's start and the
  // last output's end delimit it; clamped to the image and to what the plan sized the LDS for
  int x0 = ox0, x1 = ox0 + tw, y0 = oy0, y1 = oy0 + th;
  if (rx) {
    const int* bl = a.bounds_x + 2 * (size_t)(ox0 + tw - 1);
    x0 = clampi(a.bounds_x[2 * (size_t)ox0], 0, a.W);
    x1 = clampi(clampi(bl[0], 0, a.W) + clampi(bl[1], 0, a.ksize_x), x0, min(a.W, x0 + P.span_x));
  }
  if (ry) {
    const int* bl = a.bounds_y + 2 * (size_t)(oy0 + th - 1);
    y0 = clampi(a.bounds_y[2 * (size_t)oy0], 0, a.H);
    y1 = clampi(clampi(bl[0], 0, a.H) + clampi(bl[1], 0, a.ksize_y), y0, min(a.H, y0 + P.span_y));
  }
  if (rx) {
    for (int i = tid; i < tw; i += IP_THREADS) {
      const int* b = a.bounds_x + 2 * (size_t)(ox0 + i);
      const int first = clampi(b[0], x0, x1);
      bx[2 * i] = first - x0;
      bx[2 * i + 1] = clampi(b[1], 0, min(a.ksize_x, x1 - first));
    }
    const int* src = a.coef_x + (size_t)ox0 * a.ksize_x;
    for (int i = tid; i < tw * a.ksize_x; i += IP_THREADS) cx[i] = src[i];
  }
  if (ry) {
    for (int i = tid; i < th; i += IP_THREADS) {
      const int* b = a.bounds_y + 2 * (size_t)(oy0 + i);
      const int first = clampi(b[0], y0, y1);
      by[2 * i] = first - y0;
      by[2 * i + 1] = clampi(b[1], 0, min(a.ksize_y, y1 - first));
    }
    const int* src = a.coef_y + (size_t)oy0 * a.ksize_y;
    for (int i = tid; i < th * a.ksize_y; i += IP_THREADS) cy[i] = src[i];
  }

  // ---- source rows -> LDS -> horizontal pass -> intermediate, R rows at a time
  const unsigned char* img = a.x + (size_t)n * (size_t)a.image_stride + (size_t)x0 * ps + cbase;
  const int seg = x1 > x0 ? (x1 - x0 - 1) * ps + ci : 0;     // bytes of a row this tile reads: up to the last channel it uses
  const int ndw = P.lrow >> 2;
  for (int r0 = y0; r0 < y1; r0 += P.chunk_rows) {
    const int rows = min(P.chunk_rows, y1 - r0);
    __syncthreads();                                          // tables staged / the previous chunk's pass is done with `stage`
    for (int idx = tid; idx < rows * ndw; idx += IP_THREADS) {
      const int r = idx / ndw, k = idx - r * ndw;
      const unsigned char* g = img + (size_t)(r0 + r) * (size_t)a.row_stride;
      const int mis = (int)((uintptr_t)g & 3);                // the LDS copy keeps the global address' low two bits: dword k of the
      const unsigned char* ga = g - mis;                      // aligned global row lands in dword k of the LDS row
      const int lo = 4 * k, end = mis + seg;
      if (lo >= end) continue;
      unsigned char* d = stage + r * P.lrow + lo;
      if (lo >= mis && lo + 4 <= end) {
        *(uint32_t*)d = *(const uint32_t*)(ga + lo);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (lo + j >= mis && lo + j < end) d[j] = ga[lo + j];
      }
    }
    __syncthreads();
    const int per_row = tw * ci;
    for (int idx = tid; idx < rows * per_row; idx += IP_THREADS) {
      const int r = idx / per_row, j = idx - r * per_row;
      const int ox = j / ci, c = j - ox * ci;
      const unsigned char* g = img + (size_t)(r0 + r) * (size_t)a.row_stride;
      const unsigned char* s = stage + r * P.lrow + (int)((uintptr_t)g & 3) + c;
      unsigned char v;
      if (rx) {
        const int first = bx[2 * ox], cnt = bx[2 * ox + 1];
        const int* k = cx + ox * a.ksize_x;
        const unsigned char* sp = s + first * ps;
        uint32_t acc = 1u << 21;
        for (int x = 0; x < cnt; ++x) acc += (uint32_t)sp[x * ps] * (uint32_t)k[x];
        v = clip8(acc);
      } else {
        v = s[ox * ps];
      }
      inter[(r0 - y0 + r) * P.irow + j] = v;
    }
  }
  __syncthreads();

  // ---- vertical pass over the intermediate
  {
    const int per_row = tw * ci;
    for (int idx = tid; idx < th * per_row; idx += IP_THREADS) {
      const int oy = idx / per_row, j = idx - oy * per_row;
      unsigned char v;
      if (ry) {
        const int first = by[2 * oy], cnt = by[2 * oy + 1];
        const int* k = cy + oy * a.ksize_y;
        const unsigned char* sp = inter + first * P.irow + j;
        uint32_t acc = 1u << 21;
        for (int y = 0; y < cnt; ++y) acc += (uint32_t)sp[y * P.irow] * (uint32_t)k[y];
        v = clip8(acc);
      } else {
        v = oy < y1 - y0 ? inter[oy * P.irow + j] : 0;
      }
      outt[oy * P.irow + j] = v;
    }
  }
  __syncthreads();
  return outt;
}

template <int CI>
__global__ __launch_bounds__(IP_THREADS) void image_preprocess_kernel(const pd_image_preprocess_args a, const ip_plan P) {
#pragma clang fp contract(off)      // ToTensor / Normalize are separate fp32 div, sub, div torch ops: keep them separate IEEE operations
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int slot = a.out_index ? a.out_index[n] : n;
  if (slot < 0 || slot >= a.out_slots) return;       // (uniform over the workgroup)
  const int ox0 = blockIdx.x * IP_TOW, oy0 = blockIdx.y * IP_TOH;
  const int tw = min(IP_TOW, a.OW - ox0), th = min(IP_TOH, a.OH - oy0);
  const unsigned char* const outt = ip_resample_tile<CI>(a, P, smem, n, 0, CI, ox0, oy0, tw, th);

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

// pd_image_preprocess_bands: C independent bands in, C bands out.  A workgroup owns one tile of one GROUP of `cg` consecutive bands of one
// image (blockIdx.z = image * groups + group): the intermediate of a tile grows with the bands it carries, and the host picks the widest
// group that fits the LDS budget (all C bands at the shapes of the RGB entry; fewer for many bands under a steep down-scale).
__global__ __launch_bounds__(IP_THREADS) void image_preprocess_bands_kernel(const pd_image_preprocess_bands_args a, const ip_plan P, const int cg,
                                                                            const int groups) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, n = blockIdx.z / groups, cbase = (blockIdx.z - n * groups) * cg;
  const int slot = a.out_index ? a.out_index[n] : n;
  if (slot < 0 || slot >= a.out_slots) return;       // (uniform over the workgroup)
  const int ci = min(cg, a.C - cbase);
  const int ox0 = blockIdx.x * IP_TOW, oy0 = blockIdx.y * IP_TOH;
  const int tw = min(IP_TOW, a.OW - ox0), th = min(IP_TOH, a.OH - oy0);
  const unsigned char* const outt = ip_resample_tile<0>(a, P, smem, n, cbase, ci, ox0, oy0, tw, th);

  if (a.y_u8) {                      // uint8 NHWC [slot][OH][OW][C]: this group's ci bytes of every pixel of the tile
    const int per_row = tw * ci;
    for (int idx = tid; idx < th * per_row; idx += IP_THREADS) {
      const int oy = idx / per_row, j = idx - oy * per_row;
      const int ox = j / ci, c = j - ox * ci;
      a.y_u8[(((size_t)slot * a.OH + (oy0 + oy)) * a.OW + (ox0 + ox)) * a.C + cbase + c] = outt[oy * P.irow + j];
    }
  }
  if (a.y_f32) {                     // float32 NCHW [slot][C][OH][OW], mirrored per flips[n]
    const int flip = a.flips ? a.flips[n] : 0;
    const int per_ch = th * tw;
    for (int idx = tid; idx < ci * per_ch; idx += IP_THREADS) {
      const int c = idx / per_ch, rem = idx - c * per_ch;
      const int oy = rem / tw, ox = rem - oy * tw;
      const unsigned char v = outt[oy * P.irow + ox * ci + c];
      const float f = ((float)v / 255.0f - a.mean[cbase + c]) / a.std[cbase + c];
      const int dx = (flip & 1) ? a.OW - 1 - (ox0 + ox) : ox0 + ox;
      const int dy = (flip & 2) ? a.OH - 1 - (oy0 + oy) : oy0 + oy;
      a.y_f32[(((size_t)slot * a.C + cbase + c) * a.OH + dy) * a.OW + dx] = f;
    }
  }
}

// Pillow's kernel size of one axis: 2 * ceil(support) + 1 with support = max(in / out, 1)
static int ip_ksize(int in, int out) {
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  int c = (int)support;
  if ((double)c < support) ++c;
  return 2 * c + 1;
}

// upper bound of the source indices `tile` consecutive outputs need: first >= centre_0 - support - 0.5, end <= centre_last + support + 0.5
static int ip_span(int in, int out, int tile) {
  if (in == out) return tile < in ? tile : in;
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  const double s = (double)(tile - 1) * scale + 2.0 * support;
  int v = (int)s + 3;
  return v < in ? v : in;
}

static inline int round4(int v) { return (v + 3) & ~3; }

// The LDS layout of a workgroup that carries `ci` channels per pixel; false when it does not fit the 64 KiB ceiling.
static bool ip_make_plan(int H, int W, int OH, int OW, int pixel_stride, int ci, int kx, int ky, ip_plan* out) {
  ip_plan P;
  P.span_x = ip_span(W, OW, IP_TOW);
  P.span_y = ip_span(H, OH, IP_TOH);
  P.lrow = round4(P.span_x * pixel_stride + 4);
  P.irow = round4(IP_TOW * ci);
  P.off_cy = IP_TOW * kx * 4;
  P.off_bnd = P.off_cy + IP_TOH * ky * 4;
  P.off_inter = P.off_bnd + (IP_TOW + IP_TOH) * 2 * 4;
  P.off_out = P.off_inter + round4(P.span_y * P.irow);
  P.off_stage = round4(P.off_out + IP_TOH * P.irow + 15) & ~15;
  int R = (IP_LDS_TARGET - P.off_stage) / P.lrow;
  if (R < 4) R = (IP_LDS_MAX - P.off_stage) / P.lrow;
  if (R > 64) R = 64;
  if (R > P.span_y) R = P.span_y;
  if (R < 1) return false;
  P.chunk_rows = R;
  P.lds_bytes = P.off_stage + R * P.lrow;
  if (P.lds_bytes > IP_LDS_MAX) return false;
  *out = P;
  return true;
}

// The refusals the two entry points share (`A`: either args struct; `cin`: channels read per pixel, `cout`: channels written per pixel).
template <typename A>
static int ip_check(const A* a, const char* name, const char* cname, int cin, int cout, int max_pixel_stride) {
  PD_CHECK(a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0 && a->out_slots > 0, PD_ERR_SHAPE,
           "%s: N, H, W, OH, OW and out_slots must be positive", name);
  PD_CHECK((long long)a->H <= 32ll * a->OH && (long long)a->W <= 32ll * a->OW, PD_ERR_SHAPE,
           "%s: down-scale factor above 32 (%d x %d -> %d x %d)", name, a->H, a->W, a->OH, a->OW);
  PD_CHECK(a->pixel_stride >= cin && a->pixel_stride <= max_pixel_stride, PD_ERR_SHAPE, "%s: pixel_stride must be in [%s, %d]", name, cname,
           max_pixel_stride);
  const long long row_bytes = (long long)a->W * a->pixel_stride;
  PD_CHECK(a->row_stride >= row_bytes, PD_ERR_SHAPE, "%s: row_stride smaller than W * pixel_stride", name);
  const long long image_bytes = (long long)(a->H - 1) * a->row_stride + row_bytes;
  const long long istride = a->N == 1 ? 0 : a->image_stride;       // (not read for a single image)
  PD_CHECK(a->N == 1 || istride >= image_bytes, PD_ERR_SHAPE, "%s: image_stride smaller than one image", name);
  PD_CHECK(a->row_stride < (1ll << 32) && image_bytes < (1ll << 32) && istride < (1ll << 32) &&
               (long long)(a->N - 1) * istride + image_bytes < (1ll << 32),
           PD_ERR_SHAPE, "%s: source beyond 32-bit byte offsets in one launch", name);
  const long long out_elems = (long long)a->out_slots * cout * a->OH * a->OW;
  PD_CHECK((long long)a->OH * a->OW < (1ll << 30) && out_elems * (a->y_f32 ? 4 : 1) < (1ll << 32), PD_ERR_SHAPE,
           "%s: output beyond 32-bit byte offsets in one launch", name);
  const bool rx = a->W != a->OW, ry = a->H != a->OH;
  PD_CHECK((!rx || (a->coef_x && a->bounds_x)) && (!ry || (a->coef_y && a->bounds_y)), PD_ERR_ARG, "%s: null table of a resized axis", name);
  PD_CHECK((!rx || (a->ksize_x == ip_ksize(a->W, a->OW) && a->ksize_x <= IP_MAX_KSIZE)) &&
               (!ry || (a->ksize_y == ip_ksize(a->H, a->OH) && a->ksize_y <= IP_MAX_KSIZE)),
           PD_ERR_SHAPE, "%s: ksize must be 2 * ceil(max(in / out, 1)) + 1", name);
  PD_CHECK(a->N <= 65535 && (a->OH + IP_TOH - 1) / IP_TOH <= 65535, PD_ERR_SHAPE, "%s: more than 65535 images or row tiles in one launch", name);
  return PD_OK;
}

}  // namespace pd

using namespace pd;

extern "C" int pd_image_preprocess(const pd_image_preprocess_args* a, void* stream) {
  PD_CHECK(a != nullptr && a->x && (a->y_f32 || a->y_u8), PD_ERR_ARG, "pd_image_preprocess: null pointer (x, and at least one of y_f32 / y_u8)");
  PD_CHECK(a->Cin == 1 || a->Cin == 3, PD_ERR_ARG, "pd_image_preprocess: Cin must be 1 or 3 (got %d)", a->Cin);
  const int rc = ip_check(a, "pd_image_preprocess", "Cin", a->Cin, 3, 8);
  if (rc != PD_OK) return rc;
  const bool rx = a->W != a->OW, ry = a->H != a->OH;
  ip_plan P;
  PD_CHECK(ip_make_plan(a->H, a->W, a->OH, a->OW, a->pixel_stride, a->Cin, rx ? a->ksize_x : 0, ry ? a->ksize_y : 0, &P), PD_ERR_SHAPE,
           "pd_image_preprocess: tile does not fit the LDS budget");
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
  PD_CHECK(a->C >= 1 && a->C <= 32, PD_ERR_ARG, "pd_image_preprocess_bands: C must be in 1..32 (got %d)", a->C);
  PD_CHECK(!a->y_f32 || (a->mean && a->std), PD_ERR_ARG, "pd_image_preprocess_bands: null mean / std (fp32 [C]) with y_f32");
  const int rc = ip_check(a, "pd_image_preprocess_bands", "C", a->C, a->C, 64);
  if (rc != PD_OK) return rc;
  const bool rx = a->W != a->OW, ry = a->H != a->OH;
  const int kx = rx ? a->ksize_x : 0, ky = ry ? a->ksize_y : 0;
  // the widest band group whose workgroup keeps the 40 KiB target with chunks of >= 4 rows; failing that, the widest one that fits at all
  ip_plan P;
  int cg = 0;
  for (int c = a->C; c >= 1 && !cg; --c)
    if (ip_make_plan(a->H, a->W, a->OH, a->OW, a->pixel_stride, c, kx, ky, &P) && P.lds_bytes <= IP_LDS_TARGET && P.chunk_rows >= (P.span_y < 4 ? P.span_y : 4))
      cg = c;
  for (int c = a->C; c >= 1 && !cg; --c)
    if (ip_make_plan(a->H, a->W, a->OH, a->OW, a->pixel_stride, c, kx, ky, &P)) cg = c;
  PD_CHECK(cg > 0, PD_ERR_SHAPE, "pd_image_preprocess_bands: tile does not fit the LDS budget");
  const int groups = (a->C + cg - 1) / cg;
  PD_CHECK((long long)a->N * groups <= 65535, PD_ERR_SHAPE, "pd_image_preprocess_bands: more than 65535 (image, band group) pairs in one launch");
  const dim3 grid((unsigned)((a->OW + IP_TOW - 1) / IP_TOW), (unsigned)((a->OH + IP_TOH - 1) / IP_TOH), (unsigned)(a->N * groups));
  hipLaunchKernelGGL(image_preprocess_bands_kernel, grid, dim3(IP_THREADS), P.lds_bytes, (hipStream_t)stream, *a, P, cg, groups);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

