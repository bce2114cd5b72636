// The tiled Pillow-exact bilinear resampler under the three image entry points: pd_image_preprocess and pd_image_preprocess_bands
// (data_kernels.hip, uint8 samples) and pd_image_preprocess_bands16 (data16_kernels.hip, uint16 samples).  One tile function, one LDS
// plan, one set of argument checks, one band kernel; a sample format is a traits struct (ip_u8 / ip_u16: the sample, coefficient and
// accumulator types and the three-line tap arithmetic), so a bounds clamp or a staging fix is made once and holds for every entry.
//
// Kernel shape.  One workgroup (256 threads) owns one 8 x 32 output tile of one image (of one band group of one image):
//   1. its coefficients and (clamped, tile-relative) bounds go to LDS;
//   2. the source rows the tile's 8 output rows need are streamed global -> LDS in chunks of R rows, only the columns the tile's 32
//      output columns need, as whole dwords wherever a dword lies inside the segment (single samples at its two ragged ends, so nothing
//      outside the segment is ever read), and each chunk is run through the horizontal pass into the intermediate
//      [source rows of the tile][32 x ci samples], which stays in LDS;
//   3. the vertical pass runs over the intermediate into an 8 x 32 x ci tile of samples, which the calling kernel writes out.
// Tile size.  At the training shape (uint8, 1024 x 1280 -> 128 x 128: scale 8 x 10, 17 x 21 taps) a tile spans 74 source rows x 332 source
// columns: the intermediate is 7 KiB, the tables 3 KiB, a staged row 1 KiB.  R is chosen so that the whole workgroup stays within 40 KiB of
// the CU's 160 KiB of LDS -- four workgroups = 16 waves per CU, enough to hide the source loads behind the other workgroups' passes -- and
// 64 KiB (no opt-in attribute) is the hard ceiling, reached only near the 32 x down-scale limit on both axes.  Horizontally adjacent tiles
// share 2 x support columns (332 read for 320 owned: 4 %), vertically adjacent ones 2 x support rows (74 for 64: 14 %, re-read from L2),
// so every source byte comes from HBM about once.  A wider tile would cut the shared columns further but the 128-wide training output
// gives only 4 tiles per row as it is; a taller one doubles the intermediate at the down-scale limit (290 rows x 96 B at 8 rows).
// Every table value is clamped before it indexes anything: a malformed table gives wrong pixels, never an access outside the operands.
#pragma once
#include "pd_common.h"

namespace pd {

constexpr int IP_TOH = 8, IP_TOW = 32, IP_THREADS = 256;
constexpr int IP_MAX_KSIZE = 65;                 // 2 * 32 + 1: the 32 x down-scale limit
constexpr int IP_LDS_TARGET = 40 * 1024, IP_LDS_MAX = 64 * 1024;

// what the host derives from the shapes (the tables are device memory: the host never reads them)
struct ip_plan {
  int span_x, span_y;     // upper bounds of the source columns / rows one tile needs
  int lrow;               // bytes of one staged source row in LDS (multiple of 4, with slack for the global address' low bits)
  int irow;               // SAMPLES of one intermediate / output-tile row
  int chunk_rows;         // R
  int off_cy, off_bnd, off_inter, off_stage, off_out, lds_bytes;   // LDS layout in bytes (coef_x at 0)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Pillow's 8-bit resample (ImagingResampleHorizontal_8bpc / Vertical_8bpc): 22-bit fixed-point coefficients, accumulated with
// wrap-around (defined for any table), clip8 = >> 22 and clamp.
struct ip_u8 {
  typedef unsigned char sample;
  typedef int coef;
  typedef uint32_t acc;
  static __device__ __forceinline__ acc zero() { return 1u << 21; }
  static __device__ __forceinline__ acc tap(acc a, sample s, coef k) { return a + (uint32_t)s * (uint32_t)k; }
  static __device__ __forceinline__ sample finish(acc a) {
    const int v = (int)a >> 22;
    return (sample)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
};

// Pillow's 16bpc resample (ImagingResampleHorizontal_16bpc / Vertical_16bpc): ONE double accumulator per output sample, the product and
// the sum rounded separately (Pillow's x86-64 build has no FMA there; a 16-bit sample times a 53-bit weight is not exact, so a fused
// multiply-add changes bits): contraction is switched off in every function that holds such arithmetic.  finish is ROUND_UP + CLIP16 of
// a non-negative sum, defined for any table (a NaN or negative sum gives 0).
struct ip_u16 {
  typedef unsigned short sample;
  typedef double coef;
  typedef double acc;
  static __device__ __forceinline__ acc zero() { return 0.0; }
  static __device__ __forceinline__ acc tap(acc a, sample s, coef k) {
#pragma clang fp contract(off)
    return a + (double)s * k;
  }
  static __device__ __forceinline__ sample finish(acc a) {
#pragma clang fp contract(off)
    const double t = a + 0.5;
    if (!(t >= 0.0)) return 0;
    if (t >= 65536.0) return 65535;
    return (sample)(int)t;
  }
};

// The resample of one 8 x 32 output tile of image `n`: channels [cbase, cbase + ci) of every source pixel, each one an independent
// band of S::sample, through the horizontal and then the vertical pass (taps in ascending order into one accumulator).  `A` is any of
// the three args structs (the geometry and table fields carry the same names; the strides are BYTE strides for every sample size).
// CI > 0: the channel count at compile time (the RGB / grey entry), CI == 0: `ci_rt` channels (the band entries).  Returns the tile in
// LDS, [th][P.irow] samples with sample ox * ci + c of a row = channel cbase + c of output column ox0 + ox; ends with a barrier.
template <typename S, int CI, typename A>
__device__ __forceinline__ const typename S::sample* ip_resample_tile(const A& a, const ip_plan& P, unsigned char* smem, int n, int cbase,
                                                                      int ci_rt, int ox0, int oy0, int tw, int th) {
#pragma clang fp contract(off)
  typedef typename S::sample sample;
  typedef typename S::coef coef;
  constexpr int SB = (int)sizeof(sample);
  const int ci = CI ? CI : ci_rt;
  coef* const cx = (coef*)smem;
  coef* const cy = (coef*)(smem + P.off_cy);
  int* const bx = (int*)(smem + P.off_bnd);          // [IP_TOW][2]: first source column relative to the tile's x0, count
  int* const by = bx + 2 * IP_TOW;                   // [IP_TOH][2]
  sample* const inter = (sample*)(smem + P.off_inter);
  unsigned char* const stage = smem + P.off_stage;
  sample* const outt = (sample*)(smem + P.off_out);

  const int tid = threadIdx.x;
  const bool rx = a.W != a.OW, ry = a.H != a.OH;
  const int ps = a.pixel_stride;                     // bytes

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
    const coef* src = a.coef_x + (size_t)ox0 * a.ksize_x;
    for (int i = tid; i < tw * a.ksize_x; i += IP_THREADS) cx[i] = src[i];
  }
  if (ry) {
    for (int i = tid; i < th; i += IP_THREADS) {
      const int* b = a.bounds_y + 2 * (size_t)(oy0 + i);
      const int first = clampi(b[0], y0, y1);
      by[2 * i] = first - y0;
      by[2 * i + 1] = clampi(b[1], 0, min(a.ksize_y, y1 - first));
    }
    const coef* src = a.coef_y + (size_t)oy0 * a.ksize_y;
    for (int i = tid; i < th * a.ksize_y; i += IP_THREADS) cy[i] = src[i];
  }

  // ---- source rows -> LDS -> horizontal pass -> intermediate, R rows at a time
  const unsigned char* img = (const unsigned char*)a.x + (size_t)n * (size_t)a.image_stride + (size_t)x0 * ps + SB * cbase;
  const int seg = x1 > x0 ? (x1 - x0 - 1) * ps + SB * ci : 0;   // bytes of a row this tile reads: up to the last channel it uses
  const int ndw = P.lrow >> 2;
  for (int r0 = y0; r0 < y1; r0 += P.chunk_rows) {
    const int rows = min(P.chunk_rows, y1 - r0);
    __syncthreads();                                          // tables staged / the previous chunk's pass is done with `stage`
    for (int idx = tid; idx < rows * ndw; idx += IP_THREADS) {
      const int r = idx / ndw, k = idx - r * ndw;
      const unsigned char* g = img + (size_t)(r0 + r) * (size_t)a.row_stride;
      const int mis = (int)((uintptr_t)g & (4 - SB));         // the LDS copy keeps the (sample-aligned) global address' low bits: dword
      const unsigned char* ga = g - mis;                      // k of the aligned global row lands in dword k of the LDS row
      const int lo = 4 * k, end = mis + seg;
      if (lo >= end) continue;
      unsigned char* d = stage + r * P.lrow + lo;
      if (lo >= mis && lo + 4 <= end) {
        *(uint32_t*)d = *(const uint32_t*)(ga + lo);
      } else {                                                // a ragged end: single samples, nothing outside [g, g + seg) is read
#pragma unroll
        for (int j = 0; j < 4; j += SB)
          if (lo + j >= mis && lo + j < end) *(sample*)(d + j) = *(const sample*)(ga + lo + j);
      }
    }
    __syncthreads();
    const int per_row = tw * ci;
    for (int idx = tid; idx < rows * per_row; idx += IP_THREADS) {
      const int r = idx / per_row, j = idx - r * per_row;
      const int ox = j / ci, c = j - ox * ci;
      const unsigned char* g = img + (size_t)(r0 + r) * (size_t)a.row_stride;
      const unsigned char* s = stage + r * P.lrow + (int)((uintptr_t)g & (4 - SB)) + SB * c;
      sample v;
      if (rx) {
        const int first = bx[2 * ox], cnt = bx[2 * ox + 1];
        const coef* k = cx + ox * a.ksize_x;
        const unsigned char* sp = s + first * ps;
        typename S::acc acc = S::zero();
        for (int x = 0; x < cnt; ++x) acc = S::tap(acc, *(const sample*)(sp + x * ps), k[x]);
        v = S::finish(acc);
      } else {
        v = *(const sample*)(s + ox * ps);
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
      sample v;
      if (ry) {
        const int first = by[2 * oy], cnt = by[2 * oy + 1];
        const coef* k = cy + oy * a.ksize_y;
        const sample* sp = inter + first * P.irow + j;
        typename S::acc acc = S::zero();
        for (int y = 0; y < cnt; ++y) acc = S::tap(acc, sp[y * P.irow], k[y]);
        v = S::finish(acc);
      } else {
        v = oy < y1 - y0 ? inter[oy * P.irow + j] : 0;
      }
      outt[oy * P.irow + j] = v;
    }
  }
  __syncthreads();
  return outt;
}

// What the two band entries differ in past the resample: the raw output's field and the float tail of one sample of band `c`.
__device__ __forceinline__ unsigned char* ip_raw_out(const pd_image_preprocess_bands_args& a) { return a.y_u8; }
__device__ __forceinline__ unsigned short* ip_raw_out(const pd_image_preprocess_bands16_args& a) { return a.y_u16; }
__device__ __forceinline__ float ip_to_float(const pd_image_preprocess_bands_args& a, int c, unsigned char v) {
#pragma clang fp contract(off)      // ToTensor / Normalize are separate fp32 div, sub, div torch ops: keep them separate IEEE operations
  return ((float)v / 255.0f - a.mean[c]) / a.std[c];
}
__device__ __forceinline__ float ip_to_float(const pd_image_preprocess_bands16_args& a, int c, unsigned short v) {
#pragma clang fp contract(off)      // the window and Normalize are separate fp32 sub, sub, div, sub, div torch ops
  const float lo = a.lo[c], hi = a.hi[c];
  float f = ((float)v - lo) / (hi - lo);
  f = f < 0.0f ? 0.0f : (f > 1.0f ? 1.0f : f);                // (a NaN -- hi == lo == v -- stays a NaN, as torch.clamp keeps it)
  return (f - a.mean[c]) / a.std[c];
}

// The band entries' kernel: C independent bands in, C bands out.  A workgroup owns one tile of one GROUP of `cg` consecutive bands of one
// image (blockIdx.z = image * groups + group): the intermediate of a tile grows with the bands it carries, and the host picks the widest
// group that fits the LDS budget (all C bands at the shapes of the RGB entry; fewer for many bands under a steep down-scale).
template <typename S, typename A>
__global__ __launch_bounds__(IP_THREADS) void image_preprocess_bands_kernel(const A a, const ip_plan P, const int cg, const int groups) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, n = blockIdx.z / groups, cbase = (blockIdx.z - n * groups) * cg;
  const int slot = a.out_index ? a.out_index[n] : n;
  if (slot < 0 || slot >= a.out_slots) return;       // (uniform over the workgroup)
  const int ci = min(cg, a.C - cbase);
  const int ox0 = blockIdx.x * IP_TOW, oy0 = blockIdx.y * IP_TOH;
  const int tw = min(IP_TOW, a.OW - ox0), th = min(IP_TOH, a.OH - oy0);
  const typename S::sample* const outt = ip_resample_tile<S, 0>(a, P, smem, n, cbase, ci, ox0, oy0, tw, th);

  if (typename S::sample* const raw = ip_raw_out(a)) {   // NHWC [slot][OH][OW][C]: this group's ci samples of every pixel of the tile
    const int per_row = tw * ci;
    for (int idx = tid; idx < th * per_row; idx += IP_THREADS) {
      const int oy = idx / per_row, j = idx - oy * per_row;
      const int ox = j / ci, c = j - ox * ci;
      raw[(((size_t)slot * a.OH + (oy0 + oy)) * a.OW + (ox0 + ox)) * a.C + cbase + c] = outt[oy * P.irow + j];
    }
  }
  if (a.y_f32) {                     // float32 NCHW [slot][C][OH][OW], mirrored per flips[n]
    const int flip = a.flips ? a.flips[n] : 0;
    const int per_ch = th * tw;
    for (int idx = tid; idx < ci * per_ch; idx += IP_THREADS) {
      const int c = idx / per_ch, rem = idx - c * per_ch;
      const int oy = rem / tw, ox = rem - oy * tw;
      const float f = ip_to_float(a, cbase + c, outt[oy * P.irow + ox * ci + c]);
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

// The LDS layout of a workgroup that carries `ci` channels per pixel, for samples of `sample_bytes` and table entries of `coef_bytes`;
// false when it does not fit the 64 KiB ceiling.
//   tables     (32 * kx + 8 * ky) * coef_bytes
//   bounds     (32 + 8) * 2 * 4 B
//   inter      span_y rows x 32 * ci samples
//   out tile   8 x 32 * ci samples
//   stage      R rows x (span_x * pixel_stride + 4) B, 16-byte aligned
// (Up to the 16-bit entry's arrival the uint8 layout rounded off_stage up by a further 16 bytes when the out tile already ended on a
// 16-byte boundary.  That slack was an accident; without it R can be one row larger at a boundary, and no output depends on R.)
static bool ip_make_plan(int H, int W, int OH, int OW, int pixel_stride, int ci, int kx, int ky, int sample_bytes, int coef_bytes, ip_plan* out) {
  ip_plan P;
  P.span_x = ip_span(W, OW, IP_TOW);
  P.span_y = ip_span(H, OH, IP_TOH);
  const long long lrow = ((long long)P.span_x * pixel_stride + 4 + 3) & ~3ll;
  if (lrow > IP_LDS_MAX) return false;
  P.lrow = (int)lrow;
  P.irow = IP_TOW * ci;
  P.off_cy = IP_TOW * kx * coef_bytes;
  P.off_bnd = P.off_cy + IP_TOH * ky * coef_bytes;
  P.off_inter = P.off_bnd + (IP_TOW + IP_TOH) * 2 * 4;
  P.off_out = P.off_inter + round4(P.span_y * P.irow * sample_bytes);
  P.off_stage = (P.off_out + IP_TOH * P.irow * sample_bytes + 15) & ~15;
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

// The refusals the three entry points share.  `A`: any args struct; `sb`: bytes per sample; `cin` / `cout`: channels read / written per
// pixel; `min_ps` (spelled `min_ps_name` in the message) and `max_ps`: the limits of pixel_stride, in bytes.  The alignment of x and the
// evenness of the strides can fail for 2-byte samples only (sb - 1 is the mask).
template <typename A>
static int ip_check(const A* a, const char* name, int sb, int cin, int cout, int min_ps, const char* min_ps_name, int max_ps) {
  PD_CHECK(((uintptr_t)a->x & (uintptr_t)(sb - 1)) == 0, PD_ERR_ARG, "%s: x must be %d-byte aligned", name, sb);
  PD_CHECK(a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0 && a->out_slots > 0, PD_ERR_SHAPE,
           "%s: N, H, W, OH, OW and out_slots must be positive", name);
  PD_CHECK((long long)a->H <= 32ll * a->OH && (long long)a->W <= 32ll * a->OW, PD_ERR_SHAPE,
           "%s: down-scale factor above 32 (%d x %d -> %d x %d)", name, a->H, a->W, a->OH, a->OW);
  PD_CHECK(a->pixel_stride >= min_ps && a->pixel_stride <= max_ps, PD_ERR_SHAPE, "%s: pixel_stride must be in [%s, %d] bytes (got %d)", name,
           min_ps_name, max_ps, a->pixel_stride);
  const long long istride = a->N == 1 ? 0 : a->image_stride;       // (not read for a single image)
  PD_CHECK(((a->pixel_stride | a->row_stride | istride) & (sb - 1)) == 0, PD_ERR_SHAPE,
           "%s: pixel_stride, row_stride and image_stride are byte strides of uint16 samples and must be even", name);
  const long long row_bytes = (long long)a->W * a->pixel_stride;
  PD_CHECK(a->row_stride >= row_bytes, PD_ERR_SHAPE, "%s: row_stride smaller than W * pixel_stride", name);
  const long long image_bytes = (long long)(a->H - 1) * a->row_stride + row_bytes;
  PD_CHECK(a->N == 1 || istride >= image_bytes, PD_ERR_SHAPE, "%s: image_stride smaller than one image", name);
  PD_CHECK(a->row_stride < (1ll << 32) && image_bytes < (1ll << 32) && istride < (1ll << 32) &&
               (long long)(a->N - 1) * istride + image_bytes < (1ll << 32),
           PD_ERR_SHAPE, "%s: source beyond 32-bit byte offsets in one launch", name);
  const long long out_elems = (long long)a->out_slots * cout * a->OH * a->OW;
  PD_CHECK((long long)a->OH * a->OW < (1ll << 30) && out_elems * (a->y_f32 ? 4 : sb) < (1ll << 32), PD_ERR_SHAPE,
           "%s: output beyond 32-bit byte offsets in one launch", name);
  const bool rx = a->W != a->OW, ry = a->H != a->OH;
  PD_CHECK((!rx || (a->coef_x && a->bounds_x)) && (!ry || (a->coef_y && a->bounds_y)), PD_ERR_ARG, "%s: null table of a resized axis", name);
  PD_CHECK((!rx || (a->ksize_x == ip_ksize(a->W, a->OW) && a->ksize_x <= IP_MAX_KSIZE)) &&
               (!ry || (a->ksize_y == ip_ksize(a->H, a->OH) && a->ksize_y <= IP_MAX_KSIZE)),
           PD_ERR_SHAPE, "%s: ksize must be 2 * ceil(max(in / out, 1)) + 1", name);
  PD_CHECK(a->N <= 65535 && (a->OH + IP_TOH - 1) / IP_TOH <= 65535, PD_ERR_SHAPE, "%s: more than 65535 images or row tiles in one launch", name);
  return PD_OK;
}

// The band group of a band entry: the widest one whose workgroup keeps the 40 KiB target with chunks of >= 4 rows; failing that, the
// widest one that fits at all.  Returns the group's width with its plan in *P, or 0 when not even one band fits.
static int ip_pick_band_group(int H, int W, int OH, int OW, int pixel_stride, int C, int kx, int ky, int sample_bytes, int coef_bytes, ip_plan* P) {
  for (int c = C; c >= 1; --c)
    if (ip_make_plan(H, W, OH, OW, pixel_stride, c, kx, ky, sample_bytes, coef_bytes, P) && P->lds_bytes <= IP_LDS_TARGET &&
        P->chunk_rows >= (P->span_y < 4 ? P->span_y : 4))
      return c;
  for (int c = C; c >= 1; --c)
    if (ip_make_plan(H, W, OH, OW, pixel_stride, c, kx, ky, sample_bytes, coef_bytes, P)) return c;
  return 0;
}

// What the two band entries do once their own pointers are checked: the shared refusals, the band group, the launch.
template <typename S, typename A>
static int ip_launch_bands(const A* a, const char* name, int max_ps, void* stream) {
  constexpr int SB = (int)sizeof(typename S::sample);
  PD_CHECK(a->C >= 1 && a->C <= 32, PD_ERR_ARG, "%s: C must be in 1..32 (got %d)", name, a->C);
  PD_CHECK(!a->y_f32 || (a->mean && a->std), PD_ERR_ARG, "%s: null mean / std (fp32 [C]) with y_f32", name);
  const int rc = ip_check(a, name, SB, a->C, a->C, SB * a->C, SB == 1 ? "C" : "2 * C", max_ps);
  if (rc != PD_OK) return rc;
  const bool rx = a->W != a->OW, ry = a->H != a->OH;
  ip_plan P;
  const int cg = ip_pick_band_group(a->H, a->W, a->OH, a->OW, a->pixel_stride, a->C, rx ? a->ksize_x : 0, ry ? a->ksize_y : 0, SB,
                                    (int)sizeof(typename S::coef), &P);
  PD_CHECK(cg > 0, PD_ERR_SHAPE, "%s: tile does not fit the LDS budget", name);
  const int groups = (a->C + cg - 1) / cg;
  PD_CHECK((long long)a->N * groups <= 65535, PD_ERR_SHAPE, "%s: more than 65535 (image, band group) pairs in one launch", name);
  const dim3 grid((unsigned)((a->OW + IP_TOW - 1) / IP_TOW), (unsigned)((a->OH + IP_TOH - 1) / IP_TOH), (unsigned)(a->N * groups));
  hipLaunchKernelGGL((image_preprocess_bands_kernel<S, A>), grid, dim3(IP_THREADS), P.lds_bytes, (hipStream_t)stream, *a, P, cg, groups);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // namespace pd
