// 16-bit image stacks (plate-reader / sCMOS TIFFs: mode I;16 bands, often only 10 to 12 bits occupied).
//   pd_image_preprocess_bands16   pd_image_preprocess_bands (data_kernels.hip) for uint16 sources: Pillow's 16bpc bilinear resample bit for
//                                 bit, then an intensity window [lo, hi] -> [0, 1], Normalize and flips.
//   pd_band_histogram16           exact per-band value counts (what the window's percentiles are read from).
//   pd_postproc_bands16           the way back: float32 NCHW -> uint16 NHWC in the source's range.
// The 8-bit kernels are not touched: this file shares their TILING (8 x 32 output tiles, tables and clamped bounds in LDS, source rows
// streamed in chunks, the intermediate kept in LDS, band groups when C bands do not fit) and none of their code.
//
// Resample arithmetic (ImagingResampleHorizontal_16bpc / Vertical_16bpc): per output sample ONE double accumulator, ss = 0.0, then
// ss = ss + (double)src[first + k] * coef[k] for k in order -- the product and the sum are rounded separately (Pillow's x86-64 build has no
// FMA there; a 16-bit sample times a 53-bit weight is not exact, so a fused multiply-add changes bits): contraction is switched off in every function that
// holds such arithmetic, and the kernels' ISA holds no v_fma_f64.  out = clamp((int)(ss + 0.5), 0, 65535).  Horizontal pass first INTO uint16, then the
// vertical pass; an axis whose size does not change is skipped.
//
// LDS plan of a resample workgroup (256 threads, one 8 x 32 tile of one band group of one image), re-derived for 8-byte table entries and
// 2-byte samples:
//   tables     (32 * ksize_x + 8 * ksize_y) * 8 B   20.3 KiB at the 32 x limit on both axes (65 taps), 3.4 KiB at 1080 -> 256 (11 taps)
//   bounds     (32 + 8) * 2 * 4 B
//   inter      span_y rows x 32 * ci samples x 2 B   span_y <= 291 rows: 18.2 KiB for ONE band at the limit, 12.5 KiB for five at 1080 -> 256
//   out tile   8 x 32 * ci x 2 B
//   stage      R rows x (span_x * pixel_stride + 4) B
// R is the largest chunk that keeps the workgroup within 40 KiB (four workgroups = 16 waves per CU) and 64 KiB is the ceiling; the band
// group ci is the widest that meets the target with R >= 4, failing that the widest that fits at all.  At the limit on both axes one band
// takes 39.3 KiB before staging, so R rows of 2.1 KiB come out of the 64 KiB ceiling (R = 11, 62.1 KiB in all); five bands at
// 1080 -> 256 take 18.8 KiB before staging and R = 15 rows of 1.4 KiB: 39.6 KiB.
// Every table value is clamped before it indexes anything: a malformed table gives wrong samples, never an access outside the operands.
#include "pd_common.h"

namespace pd {

constexpr int I16_TOH = 8, I16_TOW = 32, I16_THREADS = 256;
constexpr int I16_MAX_KSIZE = 65;                 // 2 * 32 + 1: the 32 x down-scale limit
constexpr int I16_LDS_TARGET = 40 * 1024, I16_LDS_MAX = 64 * 1024;

struct i16_plan {
  int span_x, span_y;     // upper bounds of the source columns / rows one tile needs
  int lrow;               // bytes of one staged source row in LDS (multiple of 4; 2 bytes of slack for bit 1 of the global address)
  int irow;               // SAMPLES of one intermediate / output-tile row
  int chunk_rows;         // R
  int off_cy, off_bnd, off_inter, off_stage, off_out, lds_bytes;   // LDS layout in bytes (coef_x at 0)
};

__device__ __forceinline__ int i16_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Pillow's ROUND_UP + CLIP16 of a non-negative sum; defined for any table (a NaN or negative sum gives 0)
__device__ __forceinline__ unsigned short i16_round_clip(double ss) {
#pragma clang fp contract(off)
  const double t = ss + 0.5;
  if (!(t >= 0.0)) return 0;
  if (t >= 65536.0) return 65535;
  return (unsigned short)(int)t;
}

// The resample of one 8 x 32 output tile of image `n`: bands [cbase, cbase + ci) of every source pixel through the horizontal and then
// the vertical pass.  Returns the tile in LDS, [th][P.irow] samples with sample ox * ci + c of a row = band cbase + c of output column
// ox0 + ox; ends with a barrier.
__device__ __forceinline__ const unsigned short* i16_resample_tile(const pd_image_preprocess_bands16_args& a, const i16_plan& P, unsigned char* smem,
                                                                   int n, int cbase, int ci, int ox0, int oy0, int tw, int th) {
#pragma clang fp contract(off)
  double* const cx = (double*)smem;
  double* const cy = (double*)(smem + P.off_cy);
  int* const bx = (int*)(smem + P.off_bnd);          // [I16_TOW][2]: first source column relative to the tile's x0, count
  int* const by = bx + 2 * I16_TOW;                  // [I16_TOH][2]
  unsigned short* const inter = (unsigned short*)(smem + P.off_inter);
  unsigned char* const stage = smem + P.off_stage;
  unsigned short* const outt = (unsigned short*)(smem + P.off_out);

  const int tid = threadIdx.x;
  const bool rx = a.W != a.OW, ry = a.H != a.OH;
  const int ps = a.pixel_stride;                     // bytes

  // the tile's source window [x0, x1) x [y0, y1): the bounds are monotone in the output index; clamped to the image and to what the plan
  // sized the LDS for
  int x0 = ox0, x1 = ox0 + tw, y0 = oy0, y1 = oy0 + th;
  if (rx) {
    const int* bl = a.bounds_x + 2 * (size_t)(ox0 + tw - 1);
    x0 = i16_clampi(a.bounds_x[2 * (size_t)ox0], 0, a.W);
    x1 = i16_clampi(i16_clampi(bl[0], 0, a.W) + i16_clampi(bl[1], 0, a.ksize_x), x0, min(a.W, x0 + P.span_x));
  }
  if (ry) {
    const int* bl = a.bounds_y + 2 * (size_t)(oy0 + th - 1);
    y0 = i16_clampi(a.bounds_y[2 * (size_t)oy0], 0, a.H);
    y1 = i16_clampi(i16_clampi(bl[0], 0, a.H) + i16_clampi(bl[1], 0, a.ksize_y), y0, min(a.H, y0 + P.span_y));
  }
  if (rx) {
    for (int i = tid; i < tw; i += I16_THREADS) {
      const int* b = a.bounds_x + 2 * (size_t)(ox0 + i);
      const int first = i16_clampi(b[0], x0, x1);
      bx[2 * i] = first - x0;
      bx[2 * i + 1] = i16_clampi(b[1], 0, min(a.ksize_x, x1 - first));
    }
    const double* src = a.coef_x + (size_t)ox0 * a.ksize_x;
    for (int i = tid; i < tw * a.ksize_x; i += I16_THREADS) cx[i] = src[i];
  }
  if (ry) {
    for (int i = tid; i < th; i += I16_THREADS) {
      const int* b = a.bounds_y + 2 * (size_t)(oy0 + i);
      const int first = i16_clampi(b[0], y0, y1);
      by[2 * i] = first - y0;
      by[2 * i + 1] = i16_clampi(b[1], 0, min(a.ksize_y, y1 - first));
    }
    const double* src = a.coef_y + (size_t)oy0 * a.ksize_y;
    for (int i = tid; i < th * a.ksize_y; i += I16_THREADS) cy[i] = src[i];
  }

  // ---- source rows -> LDS -> horizontal pass -> intermediate, R rows at a time
  const unsigned char* img = (const unsigned char*)a.x + (size_t)n * (size_t)a.image_stride + (size_t)x0 * ps + 2 * cbase;
  const int seg = x1 > x0 ? (x1 - x0 - 1) * ps + 2 * ci : 0;   // bytes of a row this tile reads: up to the last band it uses (even)
  const int ndw = P.lrow >> 2;
  for (int r0 = y0; r0 < y1; r0 += P.chunk_rows) {
    const int rows = min(P.chunk_rows, y1 - r0);
    __syncthreads();                                          // tables staged / the previous chunk's pass is done with `stage`
    for (int idx = tid; idx < rows * ndw; idx += I16_THREADS) {
      const int r = idx / ndw, k = idx - r * ndw;
      const unsigned char* g = img + (size_t)(r0 + r) * (size_t)a.row_stride;
      const int mis = (int)((uintptr_t)g & 2);                // the LDS copy keeps bit 1 of the (even) global address: dword k of the
      const unsigned char* ga = g - mis;                      // aligned global row lands in dword k of the LDS row
      const int lo = 4 * k, end = mis + seg;
      if (lo >= end) continue;
      unsigned char* d = stage + r * P.lrow + lo;
      if (lo >= mis && lo + 4 <= end) {
        *(uint32_t*)d = *(const uint32_t*)(ga + lo);
      } else {                                                // a ragged end: single samples, nothing outside [g, g + seg) is read
#pragma unroll
        for (int j = 0; j < 4; j += 2)
          if (lo + j >= mis && lo + j < end) *(unsigned short*)(d + j) = *(const unsigned short*)(ga + lo + j);
      }
    }
    __syncthreads();
    const int per_row = tw * ci;
    for (int idx = tid; idx < rows * per_row; idx += I16_THREADS) {
      const int r = idx / per_row, j = idx - r * per_row;
      const int ox = j / ci, c = j - ox * ci;
      const unsigned char* g = img + (size_t)(r0 + r) * (size_t)a.row_stride;
      const unsigned char* s = stage + r * P.lrow + (int)((uintptr_t)g & 2) + 2 * c;
      unsigned short v;
      if (rx) {
        const int first = bx[2 * ox], cnt = bx[2 * ox + 1];
        const double* k = cx + ox * a.ksize_x;
        const unsigned char* sp = s + first * ps;
        double ss = 0.0;
        for (int x = 0; x < cnt; ++x) ss = ss + (double)*(const unsigned short*)(sp + x * ps) * k[x];
        v = i16_round_clip(ss);
      } else {
        v = *(const unsigned short*)(s + ox * ps);
      }
      inter[(r0 - y0 + r) * P.irow + j] = v;
    }
  }
  __syncthreads();

  // ---- vertical pass over the intermediate
  {
    const int per_row = tw * ci;
    for (int idx = tid; idx < th * per_row; idx += I16_THREADS) {
      const int oy = idx / per_row, j = idx - oy * per_row;
      unsigned short v;
      if (ry) {
        const int first = by[2 * oy], cnt = by[2 * oy + 1];
        const double* k = cy + oy * a.ksize_y;
        const unsigned short* sp = inter + first * P.irow + j;
        double ss = 0.0;
        for (int y = 0; y < cnt; ++y) ss = ss + (double)sp[y * P.irow] * k[y];
        v = i16_round_clip(ss);
      } else {
        v = oy < y1 - y0 ? inter[oy * P.irow + j] : 0;
      }
      outt[oy * P.irow + j] = v;
    }
  }
  __syncthreads();
  return outt;
}

// A workgroup owns one tile of one GROUP of `cg` consecutive bands of one image (blockIdx.z = image * groups + group).
__global__ __launch_bounds__(I16_THREADS) void image_preprocess_bands16_kernel(const pd_image_preprocess_bands16_args a, const i16_plan P, const int cg,
                                                                              const int groups) {
#pragma clang fp contract(off)      // the window and Normalize are separate fp32 sub, sub, div, sub, div torch ops: keep them separate IEEE operations
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, n = blockIdx.z / groups, cbase = (blockIdx.z - n * groups) * cg;
  const int slot = a.out_index ? a.out_index[n] : n;
  if (slot < 0 || slot >= a.out_slots) return;       // (uniform over the workgroup)
  const int ci = min(cg, a.C - cbase);
  const int ox0 = blockIdx.x * I16_TOW, oy0 = blockIdx.y * I16_TOH;
  const int tw = min(I16_TOW, a.OW - ox0), th = min(I16_TOH, a.OH - oy0);
  const unsigned short* const outt = i16_resample_tile(a, P, smem, n, cbase, ci, ox0, oy0, tw, th);

  if (a.y_u16) {                     // uint16 NHWC [slot][OH][OW][C]: this group's ci samples of every pixel of the tile
    const int per_row = tw * ci;
    for (int idx = tid; idx < th * per_row; idx += I16_THREADS) {
      const int oy = idx / per_row, j = idx - oy * per_row;
      const int ox = j / ci, c = j - ox * ci;
      a.y_u16[(((size_t)slot * a.OH + (oy0 + oy)) * a.OW + (ox0 + ox)) * a.C + cbase + c] = outt[oy * P.irow + j];
    }
  }
  if (a.y_f32) {                     // float32 NCHW [slot][C][OH][OW], mirrored per flips[n]
    const int flip = a.flips ? a.flips[n] : 0;
    const int per_ch = th * tw;
    for (int idx = tid; idx < ci * per_ch; idx += I16_THREADS) {
      const int c = idx / per_ch, rem = idx - c * per_ch;
      const int oy = rem / tw, ox = rem - oy * tw;
      const unsigned short v = outt[oy * P.irow + ox * ci + c];
      const float lo = a.lo[cbase + c], hi = a.hi[cbase + c];
      float f = ((float)v - lo) / (hi - lo);
      f = f < 0.0f ? 0.0f : (f > 1.0f ? 1.0f : f);            // (a NaN -- hi == lo == v -- stays a NaN, as torch.clamp keeps it)
      f = (f - a.mean[cbase + c]) / a.std[cbase + c];
      const int dx = (flip & 1) ? a.OW - 1 - (ox0 + ox) : ox0 + ox;
      const int dy = (flip & 2) ? a.OH - 1 - (oy0 + oy) : oy0 + oy;
      a.y_f32[(((size_t)slot * a.C + cbase + c) * a.OH + dy) * a.OW + dx] = f;
    }
  }
}

// Pillow's kernel size of one axis: 2 * ceil(support) + 1 with support = max(in / out, 1)
static int i16_ksize(int in, int out) {
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  int c = (int)support;
  if ((double)c < support) ++c;
  return 2 * c + 1;
}

// upper bound of the source indices `tile` consecutive outputs need: first >= centre_0 - support - 0.5, end <= centre_last + support + 0.5
static int i16_span(int in, int out, int tile) {
  if (in == out) return tile < in ? tile : in;
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  const double s = (double)(tile - 1) * scale + 2.0 * support;
  int v = (int)s + 3;
  return v < in ? v : in;
}

static inline int i16_round4(int v) { return (v + 3) & ~3; }

// The LDS layout of a workgroup that carries `ci` bands per pixel; false when it does not fit the 64 KiB ceiling.
static bool i16_make_plan(int H, int W, int OH, int OW, int pixel_stride, int ci, int kx, int ky, i16_plan* out) {
  i16_plan P;
  P.span_x = i16_span(W, OW, I16_TOW);
  P.span_y = i16_span(H, OH, I16_TOH);
  const long long lrow = ((long long)P.span_x * pixel_stride + 4 + 3) & ~3ll;
  if (lrow > I16_LDS_MAX) return false;
  P.lrow = (int)lrow;
  P.irow = I16_TOW * ci;
  P.off_cy = I16_TOW * kx * 8;
  P.off_bnd = P.off_cy + I16_TOH * ky * 8;
  P.off_inter = P.off_bnd + (I16_TOW + I16_TOH) * 2 * 4;
  P.off_out = P.off_inter + i16_round4(P.span_y * P.irow * 2);
  P.off_stage = (P.off_out + I16_TOH * P.irow * 2 + 15) & ~15;
  int R = (I16_LDS_TARGET - P.off_stage) / P.lrow;
  if (R < 4) R = (I16_LDS_MAX - P.off_stage) / P.lrow;
  if (R > 64) R = 64;
  if (R > P.span_y) R = P.span_y;
  if (R < 1) return false;
  P.chunk_rows = R;
  P.lds_bytes = P.off_stage + R * P.lrow;
  if (P.lds_bytes > I16_LDS_MAX) return false;
  *out = P;
  return true;
}

// ---- pd_band_histogram16 -------------------------------------------------------------------------------------------------------------
// A band's whole histogram is 65536 x 4 B = 256 KiB: more than a CU's LDS.  With 16-BIT counters it is 128 KiB and fits, and a 16-bit
// counter cannot overflow when the workgroup counts at most 65535 samples.  So: one workgroup (1024 threads, 128 KiB of LDS, one per CU)
// counts ONE band of a chunk of 64512 pixels (63 rounds of 1024) with LDS atomics -- dword d holds bin d in its low half and bin
// d + 32768 in its high half, so a flush lane adds to two CONTIGUOUS runs of `counts` -- then adds its non-zero bins to the global
// histogram (integer atomics: exact, order-independent).  The global atomics are at most min(chunk, 65536) per workgroup and shrink with
// the number of distinct values (12-bit data: 1 in 16 samples).
// Contention worst case, the all-equal image: 64 lanes adding to one LDS word serialise, so a wave whose valid lanes all hold one value
// (a run of background) adds its lane count once, from one lane.
constexpr int H16_THREADS = 1024, H16_UNROLL = 9, H16_CHUNK = 7 * H16_UNROLL * H16_THREADS, H16_LDS = 32768 * 4;
static_assert(H16_CHUNK <= 65535, "a 16-bit counter must hold a whole chunk");

__global__ __launch_bounds__(H16_THREADS) void band_histogram16_kernel(const pd_band_histogram16_args a, const unsigned total, const int flat) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint32_t* const h = (uint32_t*)smem;
  const int tid = threadIdx.x, lane = tid & 63, c = blockIdx.y;
  for (int i = tid; i < H16_LDS / 16; i += H16_THREADS) ((uint4*)h)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  const unsigned p0 = blockIdx.x * (unsigned)H16_CHUNK;                 // < total < 2^32
  const unsigned cnt = total - p0 < (unsigned)H16_CHUNK ? total - p0 : (unsigned)H16_CHUNK;
  const unsigned hw = (unsigned)a.H * (unsigned)a.W, w = (unsigned)a.W;
  const unsigned char* const base = (const unsigned char*)a.x + 2 * c;
  // H16_UNROLL loads in flight per lane before the first one is counted (one at a time, a wave waits a whole L2 round trip per sample).
  // Every load is unconditional, from an index clamped into the chunk (cnt >= 1); `valid` masks what lies past its end.
  for (unsigned off = 0; off < cnt; off += H16_THREADS * H16_UNROLL) {  // (uniform trip count: the ballots below see whole waves)
    unsigned v[H16_UNROLL];
#pragma unroll
    for (int u = 0; u < H16_UNROLL; ++u) {
      const unsigned i = off + (unsigned)u * H16_THREADS + tid;
      const unsigned p = p0 + (i < cnt ? i : cnt - 1);
      size_t byte;
      if (flat) {
        byte = (size_t)p * (size_t)a.pixel_stride;
      } else {
        const unsigned n = p / hw, rem = p - n * hw, y = rem / w, x = rem - y * w;
        byte = (size_t)n * (size_t)a.image_stride + (size_t)y * (size_t)a.row_stride + (size_t)x * (size_t)a.pixel_stride;
      }
      v[u] = *(const unsigned short*)(base + byte);
    }
#pragma unroll
    for (int u = 0; u < H16_UNROLL; ++u) {
      const bool valid = off + (unsigned)u * H16_THREADS + tid < cnt;
      const unsigned long long act = __ballot(valid);
      if (act != 0ull) {
        const int leader = __ffsll((long long)act) - 1;
        const unsigned v0 = (unsigned)__shfl((int)v[u], leader);
        const unsigned long long same = __ballot(valid && v[u] == v0);
        if (same == act) {
          if (lane == leader) atomicAdd(&h[v0 & 32767u], (unsigned)__popcll(act) << ((v0 >> 15) << 4));
        } else if (valid) {
          atomicAdd(&h[v[u] & 32767u], 1u << ((v[u] >> 15) << 4));
        }
      }
    }
  }
  __syncthreads();
  unsigned int* const out = a.counts + (size_t)c * 65536;
  for (int d = tid; d < 32768; d += H16_THREADS) {
    const uint32_t word = h[d];
    const unsigned lo = word & 0xffffu, hi = word >> 16;
    if (lo) atomicAdd(out + d, lo);
    if (hi) atomicAdd(out + 32768 + d, hi);
  }
}

// ---- pd_postproc_bands16 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void postproc_bands16_kernel(const pd_postproc_bands16_args a, const long long total) {
#pragma clang fp contract(off)
  const long long hw = (long long)a.H * a.W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % a.C);
    const long long pix = i / a.C, n = pix / hw, r = pix - n * hw;
    const float x = a.x[(n * a.C + c) * hw + r];
    float f = x * a.std[c] + a.mean[c];                       // two roundings (contraction is off)
    f = !(f >= 0.0f) ? 0.0f : (f > 1.0f ? 1.0f : f);          // NaN -> 0
    const float lo = a.lo[c];
    const float v = rintf(f * (a.hi[c] - lo) + lo);
    a.y[i] = (unsigned short)(!(v >= 0.0f) ? 0 : (v > 65535.0f ? 65535 : (int)v));
  }
}

}  // namespace pd

using namespace pd;

extern "C" int pd_image_preprocess_bands16(const pd_image_preprocess_bands16_args* a, void* stream) {
  const char* const name = "pd_image_preprocess_bands16";
  PD_CHECK(a != nullptr && a->x && (a->y_f32 || a->y_u16), PD_ERR_ARG, "%s: null pointer (args, x, and at least one of y_f32 / y_u16)", name);
  PD_CHECK(a->C >= 1 && a->C <= 32, PD_ERR_ARG, "%s: C must be in 1..32 (got %d)", name, a->C);
  PD_CHECK(!a->y_f32 || (a->lo && a->hi), PD_ERR_ARG, "%s: null lo / hi (fp32 [C], the intensity window) with y_f32", name);
  PD_CHECK(!a->y_f32 || (a->mean && a->std), PD_ERR_ARG, "%s: null mean / std (fp32 [C]) with y_f32", name);
  PD_CHECK(((uintptr_t)a->x & 1) == 0, PD_ERR_ARG, "%s: x must be 2-byte aligned", name);
  PD_CHECK(a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0 && a->out_slots > 0, PD_ERR_SHAPE,
           "%s: N, H, W, OH, OW and out_slots must be positive", name);
  PD_CHECK((long long)a->H <= 32ll * a->OH && (long long)a->W <= 32ll * a->OW, PD_ERR_SHAPE,
           "%s: down-scale factor above 32 (%d x %d -> %d x %d)", name, a->H, a->W, a->OH, a->OW);
  PD_CHECK(a->pixel_stride >= 2 * a->C && a->pixel_stride <= 128, PD_ERR_SHAPE, "%s: pixel_stride must be in [2 * C, 128] bytes (got %d)", name,
           a->pixel_stride);
  PD_CHECK((a->pixel_stride & 1) == 0 && (a->row_stride & 1) == 0 && (a->N == 1 || (a->image_stride & 1) == 0), PD_ERR_SHAPE,
           "%s: pixel_stride, row_stride and image_stride are byte strides of uint16 samples and must be even", name);
  const long long row_bytes = (long long)a->W * a->pixel_stride;
  PD_CHECK(a->row_stride >= row_bytes, PD_ERR_SHAPE, "%s: row_stride smaller than W * pixel_stride", name);
  const long long image_bytes = (long long)(a->H - 1) * a->row_stride + row_bytes;
  const long long istride = a->N == 1 ? 0 : a->image_stride;       // (not read for a single image)
  PD_CHECK(a->N == 1 || istride >= image_bytes, PD_ERR_SHAPE, "%s: image_stride smaller than one image", name);
  PD_CHECK(a->row_stride < (1ll << 32) && image_bytes < (1ll << 32) && istride < (1ll << 32) &&
               (long long)(a->N - 1) * istride + image_bytes < (1ll << 32),
           PD_ERR_SHAPE, "%s: source beyond 32-bit byte offsets in one launch", name);
  const long long out_elems = (long long)a->out_slots * a->C * a->OH * a->OW;
  PD_CHECK((long long)a->OH * a->OW < (1ll << 30) && out_elems * (a->y_f32 ? 4 : 2) < (1ll << 32), PD_ERR_SHAPE,
           "%s: output beyond 32-bit byte offsets in one launch", name);
  const bool rx = a->W != a->OW, ry = a->H != a->OH;
  PD_CHECK((!rx || (a->coef_x && a->bounds_x)) && (!ry || (a->coef_y && a->bounds_y)), PD_ERR_ARG, "%s: null table of a resized axis", name);
  PD_CHECK((!rx || (a->ksize_x == i16_ksize(a->W, a->OW) && a->ksize_x <= I16_MAX_KSIZE)) &&
               (!ry || (a->ksize_y == i16_ksize(a->H, a->OH) && a->ksize_y <= I16_MAX_KSIZE)),
           PD_ERR_SHAPE, "%s: ksize must be 2 * ceil(max(in / out, 1)) + 1", name);
  PD_CHECK(a->N <= 65535 && (a->OH + I16_TOH - 1) / I16_TOH <= 65535, PD_ERR_SHAPE, "%s: more than 65535 images or row tiles in one launch", name);
  const int kx = rx ? a->ksize_x : 0, ky = ry ? a->ksize_y : 0;
  // the widest band group whose workgroup keeps the 40 KiB target with chunks of >= 4 rows; failing that, the widest one that fits at all
  i16_plan P;
  int cg = 0;
  for (int c = a->C; c >= 1 && !cg; --c)
    if (i16_make_plan(a->H, a->W, a->OH, a->OW, a->pixel_stride, c, kx, ky, &P) && P.lds_bytes <= I16_LDS_TARGET &&
        P.chunk_rows >= (P.span_y < 4 ? P.span_y : 4))
      cg = c;
  for (int c = a->C; c >= 1 && !cg; --c)
    if (i16_make_plan(a->H, a->W, a->OH, a->OW, a->pixel_stride, c, kx, ky, &P)) cg = c;
  PD_CHECK(cg > 0, PD_ERR_SHAPE, "%s: tile does not fit the LDS budget", name);
  const int groups = (a->C + cg - 1) / cg;
  PD_CHECK((long long)a->N * groups <= 65535, PD_ERR_SHAPE, "%s: more than 65535 (image, band group) pairs in one launch", name);
  const dim3 grid((unsigned)((a->OW + I16_TOW - 1) / I16_TOW), (unsigned)((a->OH + I16_TOH - 1) / I16_TOH), (unsigned)(a->N * groups));
  hipLaunchKernelGGL(image_preprocess_bands16_kernel, grid, dim3(I16_THREADS), P.lds_bytes, (hipStream_t)stream, *a, P, cg, groups);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_band_histogram16(const pd_band_histogram16_args* a, void* stream) {
  const char* const name = "pd_band_histogram16";
  PD_CHECK(a != nullptr && a->x && a->counts, PD_ERR_ARG, "%s: null pointer (args, x, counts)", name);
  PD_CHECK(a->C >= 1 && a->C <= 32, PD_ERR_ARG, "%s: C must be in 1..32 (got %d)", name, a->C);
  PD_CHECK(((uintptr_t)a->x & 1) == 0, PD_ERR_ARG, "%s: x must be 2-byte aligned", name);
  PD_CHECK(a->N > 0 && a->H > 0 && a->W > 0, PD_ERR_SHAPE, "%s: N, H and W must be positive", name);
  const long long total = (long long)a->N * a->H * a->W;
  PD_CHECK((long long)a->H * a->W < (1ll << 32) && total < (1ll << 32), PD_ERR_SHAPE, "%s: N * H * W must be below 2^32 (got %lld)", name, total);
  PD_CHECK(a->pixel_stride >= 2 * a->C, PD_ERR_SHAPE, "%s: pixel_stride must be at least 2 * C bytes (got %d)", name, a->pixel_stride);
  PD_CHECK((a->pixel_stride & 1) == 0 && (a->row_stride & 1) == 0 && (a->N == 1 || (a->image_stride & 1) == 0), PD_ERR_SHAPE,
           "%s: pixel_stride, row_stride and image_stride are byte strides of uint16 samples and must be even", name);
  const long long row_bytes = (long long)a->W * a->pixel_stride;
  PD_CHECK(a->row_stride >= row_bytes, PD_ERR_SHAPE, "%s: row_stride smaller than W * pixel_stride", name);
  const long long image_bytes = (long long)(a->H - 1) * a->row_stride + row_bytes;
  PD_CHECK(a->N == 1 || a->image_stride >= image_bytes, PD_ERR_SHAPE, "%s: image_stride smaller than one image", name);
  // rows that follow each other without a gap (and images likewise) are one run of pixels: no division per sample
  const int flat = a->row_stride == row_bytes && (a->N == 1 || a->image_stride == image_bytes);
  static LdsAttr attr;
  PD_CHECK(ensure_lds(attr, band_histogram16_kernel, H16_LDS), PD_ERR_LAUNCH, "%s: cannot reserve %d bytes of LDS", name, H16_LDS);
  const dim3 grid((unsigned)((total + H16_CHUNK - 1) / H16_CHUNK), (unsigned)a->C);
  hipLaunchKernelGGL(band_histogram16_kernel, grid, dim3(H16_THREADS), H16_LDS, (hipStream_t)stream, *a, (unsigned)total, flat);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_postproc_bands16(const pd_postproc_bands16_args* a, void* stream) {
  const char* const name = "pd_postproc_bands16";
  PD_CHECK(a != nullptr && a->x && a->y && a->lo && a->hi && a->mean && a->std, PD_ERR_ARG, "%s: null pointer (args, x, y, lo, hi, mean, std)", name);
  PD_CHECK(a->C >= 1 && a->C <= 32, PD_ERR_ARG, "%s: C must be in 1..32 (got %d)", name, a->C);
  PD_CHECK(a->N > 0 && a->H > 0 && a->W > 0, PD_ERR_SHAPE, "%s: N, H and W must be positive", name);
  const long long total = (long long)a->N * a->C * a->H * a->W;
  PD_CHECK(total < (1ll << 40), PD_ERR_SHAPE, "%s: more than 2^40 elements", name);
  long long blocks = (total + 255) / 256;
  if (blocks > 1 << 20) blocks = 1 << 20;
  hipLaunchKernelGGL(postproc_bands16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a, total);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
