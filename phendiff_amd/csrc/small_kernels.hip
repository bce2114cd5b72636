// Small (bandwidth / latency bound) kernels of the PhenDiff hot path: embeddings, conv_in, GroupNorm
// statistics, fused DDIM step, add_noise, post-processing, plus the C-ABI plumbing (errors, graphs, events).
#include <stdarg.h>
#include <stdio.h>
#include "pd_common.h"
#include "pd_step.h"

namespace pd {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ================================================================================================
// pd_temb: one block per (timestep, class) row.  All weights are passed TRANSPOSED ([in][out]) so that
// thread `o` streams column o with coalesced loads.
// ================================================================================================
__global__ __launch_bounds__(256) void temb_kernel(const pd_temb_args a, int skip_proj) {
  extern __shared__ float sm[];          // [c0] sincos | [tdim] h1 | [tdim] act
  float* se = sm;
  float* h1 = sm + a.c0;
  float* act = h1 + a.tdim;
  const int row = blockIdx.x, tid = threadIdx.x;
  const float t = a.timesteps[row];
  const int half = a.c0 / 2;
  const bool first = blockIdx.y == 0;    // gridDim.y > 1 (wide models): every block redoes the cheap first layer, and takes a
                                         // 256-output slice of the second; same per-output summation order either way
  for (int i = tid; i < a.c0; i += 256) {
    // get_timestep_embedding: emb = [sin | cos], flipped to [cos | sin] when flip_sin_to_cos
    const bool second = i >= half;
    const int k = second ? i - half : i;
    const float expo = (-9.210340371976184f /* -ln(10000) */ * (float)k) / ((float)half - a.freq_shift);
    const float arg = t * expf(expo);
    const bool want_sin = a.flip_sin_to_cos ? second : !second;
    se[i] = want_sin ? sinf(arg) : cosf(arg);
    if (a.feat && first) a.feat[(size_t)row * a.c0 + i] = se[i];
  }
  __syncthreads();
  for (int o = tid; o < a.tdim; o += 256) {
    float acc = a.b1[o];
    const float* w = a.w1 + o;
#pragma unroll 8
    for (int i = 0; i < a.c0; ++i) acc += w[(size_t)i * a.tdim] * se[i];
    if (a.z1 && first) a.z1[(size_t)row * a.tdim + o] = acc;
    h1[o] = silu_f(acc);
  }
  __syncthreads();
  for (int o = blockIdx.y * 256 + tid; o < a.tdim; o += 256 * gridDim.y) {
    float acc = a.b2[o];
    const float* w = a.w2 + o;
#pragma unroll 8
    for (int i = 0; i < a.tdim; ++i) acc += w[(size_t)i * a.tdim] * h1[i];
    if (a.class_emb) acc += a.class_emb[(size_t)row * a.tdim + o];
    else if (a.labels && a.class_table) acc += a.class_table[(size_t)a.labels[row] * a.tdim + o];
    if (a.emb) a.emb[(size_t)row * a.tdim + o] = acc;
    act[o] = silu_f(acc);
  }
  __syncthreads();
  if (skip_proj) return;                 // the projections run in temb_proj_kernel (wide models: one block per 256 outputs)
  for (int o = tid; o < a.proj_dim; o += 256) {
    float acc = a.bp[o];
    const float* w = a.wp + o;
#pragma unroll 8
    for (int i = 0; i < a.tdim; ++i) acc += w[(size_t)i * a.proj_dim] * act[i];
    a.proj[(size_t)row * a.proj_dim + o] = acc;
  }
}

// proj[r][o] = bp[o] + sum_i wp[i][o] * silu(emb[r][i]);  grid (ceil(rows / TEMB_R), proj_dim / 256): a block keeps TEMB_R rows
// of activations in LDS so each weight it streams serves TEMB_R rows.  Same summation order as the tail of temb_kernel, so
// both paths give identical bits.
constexpr int TEMB_R = 8;
__global__ __launch_bounds__(256) void temb_proj_kernel(const pd_temb_args a) {
  extern __shared__ float act[];         // [TEMB_R][tdim]
  const int row0 = blockIdx.x * TEMB_R, tid = threadIdx.x;
  const int nr = min(TEMB_R, a.rows - row0);
  for (int i = tid; i < TEMB_R * a.tdim; i += 256) {
    const int r = i / a.tdim;
    act[i] = r < nr ? silu_f(a.emb[(size_t)(row0 + r) * a.tdim + (i - r * a.tdim)]) : 0.f;
  }
  __syncthreads();
  const int o = blockIdx.y * 256 + tid;
  if (o >= a.proj_dim) return;
  float acc[TEMB_R];
#pragma unroll
  for (int r = 0; r < TEMB_R; ++r) acc[r] = a.bp[o];
  const float* w = a.wp + o;
#pragma unroll 4
  for (int i = 0; i < a.tdim; ++i) {
    const float wv = w[(size_t)i * a.proj_dim];
#pragma unroll
    for (int r = 0; r < TEMB_R; ++r) acc[r] += wv * act[r * a.tdim + i];
  }
#pragma unroll
  for (int r = 0; r < TEMB_R; ++r)
    if (r < nr) a.proj[(size_t)(row0 + r) * a.proj_dim + o] = acc[r];
}

// ================================================================================================
// pd_conv_in: direct 3x3 conv, Cin <= 4.  thread = (pixel, group of 8 output channels); the 8 threads of a
// pixel write one contiguous NHWC row.
// ================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void conv_in_kernel(const pd_conv_in_args a) {
  extern __shared__ float wsm[];   // [Cin*9][Cout] transposed weights
  const int nw = a.Cout * a.Cin * 9;
  for (int i = threadIdx.x; i < nw; i += 256) {
    const int co = i / (a.Cin * 9), k = i % (a.Cin * 9);
    wsm[k * a.Cout + co] = a.w[i];
  }
  __syncthreads();
  const int groups = a.Cout / 8;
  const size_t total = (size_t)a.B * a.H * a.W * groups;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int cg = (int)(gid % groups);
  const size_t pix = gid / groups;
  const int x = (int)(pix % a.W), y = (int)((pix / a.W) % a.H), n = (int)(pix / ((size_t)a.W * a.H));
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = a.bias[cg * 8 + j];
  for (int ci = 0; ci < a.Cin; ++ci) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = y + ky - 1, ix = x + kx - 1;
        float v = 0.f;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = a.x[(((size_t)n * a.Cin + ci) * a.H + iy) * a.W + ix];
        const float* wr = wsm + ((ci * 3 + ky) * 3 + kx) * a.Cout + cg * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += wr[j] * v;
      }
    }
  }
  T* dst = (T*)a.y + pix * a.Cout + cg * 8;
  store4(dst, acc[0], acc[1], acc[2], acc[3]);
  store4(dst + 4, acc[4], acc[5], acc[6], acc[7]);
}

// ================================================================================================
// pd_gn_stats: (1) per-channel partial sums over a pixel slice, coalesced 8-channel pieces, fp32 per
// thread then fp64 combine; (2) finalize: group moments in fp64 -> per-(sample, channel) scale / shift.
// ================================================================================================
// ResnetBlock2D(time_embedding_norm = "scale_shift"): y = GN(x) * (1 + s) + t with [s | t] = this resnet's time_emb_proj row --
// folded into the per-(sample, channel) affine the consumer applies: (x*sc + sh)*(1 + s) + t
__device__ __forceinline__ void gn_write_affine(const pd_gn_finalize_args& a, int n, int C, int c, float sc, float sh) {
  if (a.temb) {
    const float* row = a.temb + (size_t)n * a.temb_stride;
    const float s = 1.0f + row[c];
    sc *= s;
    sh = sh * s + row[C + c];
  }
  a.scale[(size_t)n * C + c] = sc;
  a.shift[(size_t)n * C + c] = sh;
}

template <typename T>
__global__ __launch_bounds__(256) void gn_partial_kernel(const pd_gn_stats_args a) {
  using E = Elem<T>;
  __shared__ float red[256 * 16];
  const int C = a.C0 + a.C1;
  const int PP = C / 8;                 // pieces per pixel
  const int ppi = 256 / PP;             // pixels per iteration
  const int nthr = ppi * PP;
  const int n = blockIdx.x / a.splits, split = blockIdx.x % a.splits;
  const int per = (a.HW + a.splits - 1) / a.splits;
  const int p0 = split * per, p1 = min(a.HW, p0 + per);
  const int tid = threadIdx.x;
  float s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
  if (tid < nthr) {
    const int piece = tid % PP, prow = tid / PP;
    const int c8 = piece * 8;
    const T* src; int cs, coff;
    if (c8 < a.C0) { src = (const T*)a.x0; cs = a.C0; coff = c8; }
    else           { src = (const T*)a.x1; cs = a.C1; coff = c8 - a.C0; }
    for (int p = p0 + prow; p < p1; p += ppi) {
      float v[8];
      E::unpack(E::load(src + ((size_t)n * a.HW + p) * cs + coff), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) { s[j] += v[j]; q[j] += v[j] * v[j]; }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[tid * 16 + j] = s[j]; red[tid * 16 + 8 + j] = q[j]; }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int piece = c >> 3, j = c & 7;
    double ds = 0.0, dq = 0.0;
    for (int k = 0; k < ppi; ++k) {
      const int t = k * PP + piece;
      ds += (double)red[t * 16 + j];
      dq += (double)red[t * 16 + 8 + j];
    }
    double* out = a.partial + (((size_t)n * a.splits + split) * C + c) * 2;
    out[0] = ds; out[1] = dq;
  }
}

__global__ __launch_bounds__(256) void gn_finalize_kernel(const pd_gn_stats_args a) {
  __shared__ float mean_s[64], rstd_s[64];
  const int C = a.C0 + a.C1;
  const int gs = C / a.groups;
  const int n = blockIdx.x, tid = threadIdx.x;
  if (tid < a.groups) {
    double ds = 0.0, dq = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) {
      const double* in = a.partial + (((size_t)n * a.splits + sp) * C + tid * gs) * 2;
      for (int c = 0; c < gs; ++c) { ds += in[2 * c]; dq += in[2 * c + 1]; }
    }
    const double cnt = (double)gs * (double)a.HW;
    const double mean = ds / cnt;
    double var = dq / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    mean_s[tid] = (float)mean;
    rstd_s[tid] = (float)(1.0 / sqrt(var + (double)a.eps));
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int g = c / gs;
    const float sc = rstd_s[g] * a.gamma[c];
    a.scale[(size_t)n * C + c] = sc;
    a.shift[(size_t)n * C + c] = a.beta[c] - mean_s[g] * sc;
  }
}

// pd_gn_finalize: per-tile channel sums written by pd_conv epilogues -> scale / shift.  One block per sample;
// thread (channel-in-block-of-64, tile slice) streams the tile axis with coalesced 512-B rows; fp64 combine.
// grid = (B, channel blocks): each block owns CB consecutive channels that contain only whole groups (CB = 96 is a
// multiple of every group size in the shipped models; otherwise one block takes all channels).
__global__ __launch_bounds__(1024) void gn_finalize2_kernel(const pd_gn_finalize_args a, int CB) {
  __shared__ double chs[1024], chq[1024];
  __shared__ double part[16][64][2];
  __shared__ float mean_s[64], rstd_s[64];
  const int C = a.C0 + a.C1;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int c_lo = blockIdx.y * CB, c_hi = min(C, c_lo + CB);
  const int cl = tid & 63, sl = tid >> 6;        // 64 channels x 16 tile slices
  for (int cb = c_lo; cb < c_hi; cb += 64) {
    const int c = cb + cl;
    double s = 0.0, q = 0.0;
    if (c < c_hi) {
      const bool first = c < a.C0;
      const float* st = first ? a.stats0 : a.stats1;
      const int Cs = first ? a.C0 : a.C1, T = first ? a.T0 : a.T1, cc = first ? c : c - a.C0;
      const float* base = st + ((size_t)n * T * Cs + cc) * 2;
      for (int t = sl; t < T; t += 16) {
        const float2 v = *(const float2*)(base + (size_t)t * Cs * 2);
        s += (double)v.x; q += (double)v.y;
      }
    }
    part[sl][cl][0] = s; part[sl][cl][1] = q;
    __syncthreads();
    if (sl == 0 && c < c_hi) {
      double ts = 0.0, tq = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) { ts += part[k][cl][0]; tq += part[k][cl][1]; }
      chs[c - c_lo] = ts; chq[c - c_lo] = tq;
    }
    __syncthreads();
  }
  const int gs = C / a.groups;
  const int g_lo = c_lo / gs, ng = (c_hi - c_lo) / gs;
  if (tid < ng) {
    double ds = 0.0, dq = 0.0;
    for (int c = tid * gs; c < (tid + 1) * gs; ++c) { ds += chs[c]; dq += chq[c]; }
    const double cnt = (double)gs * (double)a.HW;
    const double mean = ds / cnt;
    double var = dq / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    mean_s[tid] = (float)mean;
    rstd_s[tid] = (float)(1.0 / sqrt(var + (double)a.eps));
    if (a.mean) { a.mean[n * a.groups + g_lo + tid] = mean_s[tid]; a.rstd[n * a.groups + g_lo + tid] = rstd_s[tid]; }
  }
  __syncthreads();
  for (int c = c_lo + tid; c < c_hi; c += 1024) {
    const int g = c / gs - g_lo;
    const float sc = rstd_s[g] * a.gamma[c];
    gn_write_affine(a, n, C, c, sc, a.beta[c] - mean_s[g] * sc);
  }
}

// Many-block form for the common small groups (<= 16 channels per group): a block owns CB ~ 16 consecutive channels (whole
// groups) of one sample, 1024 threads = CBp channel lanes x 1024/CBp tile slices, so a 256-tile statistic row is 4 independent
// loads per thread instead of 16 and a launch has 4-32x more blocks than samples (the one-block-per-sample form above is
// latency-bound at 8-14 us per launch, 41 launches per UNet forward).  Same fp64 combine, fixed-order tree: deterministic.
__global__ __launch_bounds__(1024) void gn_finalize3_kernel(const pd_gn_finalize_args a, int CB, int CBp) {
  __shared__ double ps[1024], pq[1024];
  __shared__ float mean_s[16], rstd_s[16];
  const int C = a.C0 + a.C1;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int c_lo = blockIdx.y * CB, c_hi = min(C, c_lo + CB);
  const int cl = tid & (CBp - 1), sl = tid / CBp, S = 1024 / CBp;
  const int c = c_lo + cl;
  double s = 0.0, q = 0.0;
  if (cl < CB && c < c_hi) {
    const bool first = c < a.C0;
    const float* st = first ? a.stats0 : a.stats1;
    const int Cs = first ? a.C0 : a.C1, T = first ? a.T0 : a.T1, cc = first ? c : c - a.C0;
    const float* base = st + ((size_t)n * T * Cs + cc) * 2;
#pragma unroll 4
    for (int t = sl; t < T; t += S) {
      const float2 v = *(const float2*)(base + (size_t)t * Cs * 2);
      s += (double)v.x; q += (double)v.y;
    }
  }
  ps[tid] = s; pq[tid] = q;
  __syncthreads();
  for (int off = S >> 1; off > 0; off >>= 1) {
    if (sl < off) { ps[tid] += ps[tid + off * CBp]; pq[tid] += pq[tid + off * CBp]; }
    __syncthreads();
  }
  const int gs = C / a.groups;
  const int g_lo = c_lo / gs, ng = (c_hi - c_lo) / gs;
  if (tid < ng) {
    double ds = 0.0, dq = 0.0;
    for (int k = tid * gs; k < (tid + 1) * gs; ++k) { ds += ps[k]; dq += pq[k]; }
    const double cnt = (double)gs * (double)a.HW;
    const double mean = ds / cnt;
    double var = dq / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    mean_s[tid] = (float)mean;
    rstd_s[tid] = (float)(1.0 / sqrt(var + (double)a.eps));
    if (a.mean) { a.mean[n * a.groups + g_lo + tid] = mean_s[tid]; a.rstd[n * a.groups + g_lo + tid] = rstd_s[tid]; }
  }
  __syncthreads();
  if (tid < c_hi - c_lo) {
    const int cc = c_lo + tid;
    const int g = tid / gs;
    const float sc = rstd_s[g] * a.gamma[cc];
    gn_write_affine(a, n, C, cc, sc, a.beta[cc] - mean_s[g] * sc);
  }
}

// ================================================================================================
// pd_ddim_step / pd_add_noise / pd_postproc: elementwise on fp32 NCHW
// ================================================================================================
// FP contraction is OFF in ddim_step_kernel and add_noise_kernel (pd_step.h says why).  One pass: 256 threads x 4 elements.
__global__ __launch_bounds__(256) void ddim_step_kernel(const pd_ddim_step_args a) {
#pragma clang fp contract(off)
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= a.numel) return;
  const StepOperands r = step_operands(a, i0);
  float xp[4], x0v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xp[j] = ddim_step_elem(a, r.x[j], r.out[j], x0v[j]);
  store_quad(a.prev_sample, i0, r.cnt, xp);
  if (a.pred_x0) store_quad(a.pred_x0, i0, r.cnt, x0v);
}

__global__ __launch_bounds__(256) void add_noise_kernel(const pd_add_noise_args a) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.numel) return;
  const int64_t n = i / a.per_sample;
  const float sa = a.sa[n], sb = a.sb[n];
  a.out[i] = a.velocity ? (sa * a.noise[i] - sb * a.x[i]) : (sa * a.x[i] + sb * a.noise[i]);
}

__global__ __launch_bounds__(256) void postproc_kernel(const pd_postproc_args a) {
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t hw = (size_t)a.H * a.W;
  if (pix >= (size_t)a.B * hw) return;
  const size_t n = pix / hw, p = pix % hw;
  for (int c = 0; c < a.C; ++c) {
    float v = a.x[(n * a.C + c) * hw + p];
    v = fminf(fmaxf(v / 2.f + 0.5f, 0.f), 1.f);
    if (a.out_f32) a.out_f32[pix * a.C + c] = v;
    if (a.out_u8) a.out_u8[pix * a.C + c] = (uint8_t)rintf(v * 255.f);
  }
}

}  // namespace pd

using namespace pd;

extern "C" int pd_abi_version(void) { return PD_ABI_VERSION; }
extern "C" const char* pd_last_error(void) { return g_err; }

extern "C" int pd_temb(const pd_temb_args* a, void* stream) {
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_temb: null args");
  PD_CHECK(a->rows > 0 && a->c0 > 0 && a->c0 % 2 == 0 && a->tdim > 0 && a->proj_dim > 0, PD_ERR_SHAPE, "pd_temb: bad dims");
  PD_CHECK(a->timesteps && a->w1 && a->b1 && a->w2 && a->b2 && a->wp && a->bp && a->proj, PD_ERR_ARG, "pd_temb: null pointer");
  PD_CHECK(!(a->labels && a->class_emb), PD_ERR_ARG, "pd_temb: both labels and class_emb given");
  PD_CHECK(!(a->labels && !a->class_table), PD_ERR_ARG, "pd_temb: labels without class table");
  const size_t sm = (size_t)(a->c0 + 2 * a->tdim) * sizeof(float);
  PD_CHECK(sm <= 64 * 1024, PD_ERR_SHAPE, "pd_temb: tdim too large");
  // wide projection stacks (the SD UNet: 22 720 outputs of 1280 inputs per row) on few rows: spread the projections over
  // proj_dim / 256 blocks per row; needs the emb buffer as the hand-over
  const int split = a->emb != nullptr && (long long)a->proj_dim * a->tdim >= (1 << 22) && a->rows < 1024;
  hipLaunchKernelGGL(temb_kernel, dim3(a->rows, split ? (a->tdim + 255) / 256 : 1), dim3(256), sm, (hipStream_t)stream, *a, split);
  PD_LAUNCH_CHECK();
  if (split) {
    PD_CHECK((size_t)TEMB_R * a->tdim * sizeof(float) <= 64 * 1024, PD_ERR_SHAPE, "pd_temb: tdim too large for the split projection");
    hipLaunchKernelGGL(temb_proj_kernel, dim3((a->rows + TEMB_R - 1) / TEMB_R, (a->proj_dim + 255) / 256), dim3(256),
                       (size_t)TEMB_R * a->tdim * sizeof(float), (hipStream_t)stream, *a);
    PD_LAUNCH_CHECK();
  }
  return PD_OK;
}

extern "C" int pd_conv_in(const pd_conv_in_args* a, void* stream) {
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_conv_in: null args");
  PD_CHECK(a->Cin >= 1 && a->Cin <= 4 && a->Cout % 32 == 0 && a->Cout > 0, PD_ERR_SHAPE, "pd_conv_in: Cin=%d Cout=%d", a->Cin, a->Cout);
  PD_CHECK(a->B > 0 && a->H > 0 && a->W > 0 && a->x && a->w && a->bias && a->y, PD_ERR_ARG, "pd_conv_in: bad args");
  const size_t total = (size_t)a->B * a->H * a->W * (a->Cout / 8);
  const size_t sm = (size_t)a->Cout * a->Cin * 9 * sizeof(float);
  PD_CHECK(sm <= 64 * 1024, PD_ERR_SHAPE, "pd_conv_in: weights do not fit LDS");
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (a->dtype == PD_F32) hipLaunchKernelGGL(conv_in_kernel<float>, dim3(grid), dim3(256), sm, (hipStream_t)stream, *a);
  else if (a->dtype == PD_BF16) hipLaunchKernelGGL(conv_in_kernel<bf16_t>, dim3(grid), dim3(256), sm, (hipStream_t)stream, *a);
  else if (a->dtype == PD_F16) hipLaunchKernelGGL(conv_in_kernel<half_t>, dim3(grid), dim3(256), sm, (hipStream_t)stream, *a);
  else { set_error("pd_conv_in: bad dtype"); return PD_ERR_ARG; }
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_gn_stats(const pd_gn_stats_args* a, void* stream) {
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_gn_stats: null args");
  const int C = a->C0 + a->C1;
  PD_CHECK(a->B > 0 && a->HW > 0 && a->C0 > 0 && a->C0 % 32 == 0 && a->C1 % 32 == 0 && a->C1 >= 0, PD_ERR_SHAPE, "pd_gn_stats: bad shape");
  PD_CHECK(a->groups > 0 && a->groups <= 64 && C % a->groups == 0 && C / 8 <= 256, PD_ERR_SHAPE, "pd_gn_stats: groups=%d C=%d", a->groups, C);
  PD_CHECK(a->splits >= 1 && a->x0 && a->gamma && a->beta && a->partial && a->scale && a->shift, PD_ERR_ARG, "pd_gn_stats: null pointer");
  PD_CHECK((a->C1 == 0) == (a->x1 == nullptr), PD_ERR_ARG, "pd_gn_stats: x1/C1 mismatch");
  hipStream_t st = (hipStream_t)stream;
  if (a->dtype == PD_F32) hipLaunchKernelGGL(gn_partial_kernel<float>, dim3(a->B * a->splits), dim3(256), 0, st, *a);
  else if (a->dtype == PD_BF16) hipLaunchKernelGGL(gn_partial_kernel<bf16_t>, dim3(a->B * a->splits), dim3(256), 0, st, *a);
  else if (a->dtype == PD_F16) hipLaunchKernelGGL(gn_partial_kernel<half_t>, dim3(a->B * a->splits), dim3(256), 0, st, *a);
  else { set_error("pd_gn_stats: bad dtype"); return PD_ERR_ARG; }
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(a->B), dim3(256), 0, st, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_gn_finalize(const pd_gn_finalize_args* a, void* stream) {
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_gn_finalize: null args");
  const int C = a->C0 + a->C1;
  PD_CHECK(a->B > 0 && a->HW > 0 && a->C0 > 0 && a->C1 >= 0 && C <= 16384 && a->T0 > 0, PD_ERR_SHAPE, "pd_gn_finalize: bad shape (C=%d)", C);
  PD_CHECK(a->groups > 0 && a->groups <= 64 && C % a->groups == 0, PD_ERR_SHAPE, "pd_gn_finalize: groups=%d C=%d", a->groups, C);
  PD_CHECK(a->stats0 && a->gamma && a->beta && a->scale && a->shift, PD_ERR_ARG, "pd_gn_finalize: null pointer");
  PD_CHECK((a->C1 == 0) == (a->stats1 == nullptr) && (a->C1 == 0 || a->T1 > 0), PD_ERR_ARG, "pd_gn_finalize: stats1/C1 mismatch");
  PD_CHECK((a->mean == nullptr) == (a->rstd == nullptr), PD_ERR_ARG, "pd_gn_finalize: mean/rstd must be given together");
  PD_CHECK(a->temb == nullptr || a->temb_stride >= 2 * C, PD_ERR_ARG, "pd_gn_finalize: temb_stride must cover the [scale | shift] row (2*C)");
  const int gs = C / a->groups;
  PD_CHECK(gs <= 1024, PD_ERR_SHAPE, "pd_gn_finalize: %d channels per group", gs);
  if (gs <= 16) {
    const int CB3 = gs * (16 / gs);                 // <= 16 channels of whole groups per block
    int CBp = 1;
    while (CBp < CB3) CBp <<= 1;
    hipLaunchKernelGGL(gn_finalize3_kernel, dim3(a->B, (C + CB3 - 1) / CB3), dim3(1024), 0, (hipStream_t)stream, *a, CB3, CBp);
    PD_LAUNCH_CHECK();
    return PD_OK;
  }
  const int CB = gs * (gs <= 96 ? 96 / gs : 1);     // channel block of whole groups (<= 1024 channels, <= 64 groups)
  hipLaunchKernelGGL(gn_finalize2_kernel, dim3(a->B, (C + CB - 1) / CB), dim3(1024), 0, (hipStream_t)stream, *a, CB);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_ddim_step(const pd_ddim_step_args* a, void* stream) {
  const char* const who = "pd_ddim_step";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  if (const int rc = step_validate_common(a->numel, a->per_sample, a->pred_type, who, PD_ERR_ARG)) return rc;
  PD_CHECK(a->sample && a->model_out && a->prev_sample, PD_ERR_ARG, "%s: sample / model_out / prev_sample is NULL", who);
  PD_CHECK(!a->uncond_out || a->w, PD_ERR_ARG, "%s: guidance without weights", who);
  if (const int rc = step_check_aligned16({{"sample", a->sample}, {"model_out", a->model_out}, {"uncond_out", a->uncond_out},
                                           {"prev_sample", a->prev_sample}, {"pred_x0", a->pred_x0}}, who)) return rc;
  const unsigned grid = (unsigned)((a->numel + 1023) / 1024);
  hipLaunchKernelGGL(ddim_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_add_noise(const pd_add_noise_args* a, void* stream) {
  PD_CHECK(a != nullptr && a->numel > 0 && a->per_sample > 0 && a->x && a->noise && a->sa && a->sb && a->out, PD_ERR_ARG, "pd_add_noise: bad args");
  hipLaunchKernelGGL(add_noise_kernel, dim3((unsigned)((a->numel + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_zero(const pd_zero_args* a, void* stream) {
  PD_CHECK(a != nullptr && a->ptr && a->bytes > 0, PD_ERR_ARG, "pd_zero: bad args");
  PD_CHECK(hipMemsetAsync(a->ptr, 0, a->bytes, (hipStream_t)stream) == hipSuccess, PD_ERR_LAUNCH, "pd_zero: hipMemsetAsync failed");
  return PD_OK;
}

extern "C" int pd_postproc(const pd_postproc_args* a, void* stream) {
  PD_CHECK(a != nullptr && a->B > 0 && a->C > 0 && a->H > 0 && a->W > 0 && a->x && (a->out_f32 || a->out_u8), PD_ERR_ARG, "pd_postproc: bad args");
  const size_t total = (size_t)a->B * a->H * a->W;
  hipLaunchKernelGGL(postproc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

// ---- hipGraph capture of the sampling loop ------------------------------------------------------------
#define PD_HIP(call)                                                         \
  do {                                                                       \
    hipError_t e_ = (call);                                                  \
    if (e_ != hipSuccess) { set_error("%s: %s", #call, hipGetErrorString(e_)); return PD_ERR_LAUNCH; } \
  } while (0)

extern "C" int pd_graph_begin(void* stream) {
  PD_HIP(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
  return PD_OK;
}
extern "C" int pd_graph_end(void* stream, void** graph_exec_out) {
  PD_CHECK(graph_exec_out != nullptr, PD_ERR_ARG, "pd_graph_end: null out");
  hipGraph_t g = nullptr;
  PD_HIP(hipStreamEndCapture((hipStream_t)stream, &g));
  hipGraphExec_t ge = nullptr;
  hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) { set_error("hipGraphInstantiate: %s", hipGetErrorString(e)); return PD_ERR_LAUNCH; }
  *graph_exec_out = (void*)ge;
  return PD_OK;
}
extern "C" int pd_graph_launch(void* graph_exec, void* stream) {
  PD_CHECK(graph_exec != nullptr, PD_ERR_ARG, "pd_graph_launch: null graph");
  PD_HIP(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
  return PD_OK;
}
extern "C" int pd_graph_destroy(void* graph_exec) {
  if (graph_exec) PD_HIP(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
  return PD_OK;
}

extern "C" int pd_event_create(void** ev) {
  PD_CHECK(ev != nullptr, PD_ERR_ARG, "pd_event_create: null out");
  hipEvent_t e;
  PD_HIP(hipEventCreate(&e));
  *ev = (void*)e;
  return PD_OK;
}
extern "C" int pd_event_record(void* ev, void* stream) {
  PD_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
  return PD_OK;
}
extern "C" int pd_event_elapsed_ms(void* start, void* stop, float* ms) {
  PD_CHECK(ms != nullptr, PD_ERR_ARG, "pd_event_elapsed_ms: null out");
  PD_HIP(hipEventSynchronize((hipEvent_t)stop));
  PD_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return PD_OK;
}
extern "C" int pd_event_destroy(void* ev) {
  if (ev) PD_HIP(hipEventDestroy((hipEvent_t)ev));
  return PD_OK;
}
