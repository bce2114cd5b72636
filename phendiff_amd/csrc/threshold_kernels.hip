// Dynamic thresholding of DDIMScheduler (diffusers' _threshold_sample) on the device, inside a captured trajectory:
//   pd_ddim_raw_x0          the unclamped x0 of a step (guidance combine included) into a scratch buffer
//   pd_abs_quantile         out[b] = lerp(a_(lo), a_(hi), w) over |x[b][:]|: an exact per-row order statistic, no host read
//   pd_ddim_step_threshold  pd_ddim_step with  s = min(max(q[b], 1), sample_max_value),  x0 = min(max(x0, -s), s) / s  for the static clamp
//
// Which x0 is thresholded: pd_ddim_step_threshold RECOMPUTES x0 from sample / model_out (/ uncond_out) through ddim_x0_eps (pd_step.h),
// the inline function pd_ddim_raw_x0 went through, under the same contraction setting (off) and after the same guidance combine
// (step_operands, pd_step.h: one definition for every step kernel): the same IEEE operations on the same inputs, so the x0 that is
// thresholded is bit for bit the x0 whose quantile was taken, and the update does not read the scratch buffer again.  The clamp is
// threshold_limit (pd_step.h), the one pd_multistep_step applies.
//
// ---- pd_abs_quantile: most-significant-digit radix select over the 31 bits of |v| (11 + 10 + 10) -----------------------------------------
// For everything that is not a NaN the bit pattern of |v| orders like the value, so the k-th smallest key IS the order statistic.  Per
// digit: a histogram launch over (chunk, row), then a one-workgroup-per-row launch that finds the bin holding each rank and narrows the
// prefix.  The two ranks (hi in {lo, lo + 1}) are two selections: while their prefixes agree they share one histogram, from the pass where
// they part each has its own (elements are counted under the prefix they match), so both come out exact wherever the seam falls.
// A row of 3 x 256 x 256 elements is 768 KiB, more than a CU's LDS: the grid is (chunks of 8192 elements, rows); a workgroup counts its
// chunk into LDS and adds its non-zero bins to the row's histogram in the workspace with global integer atomics.  Integers only: exact,
// and independent of B, of the schedule of workgroups and of the replay.
//   LDS per workgroup: 2048 bins x 4 B = 8 KiB (pass 0: one 2048-bin histogram; passes 1, 2: two of 1024 bins) -- 20 workgroups of 4 waves
//   would fit a CU's 160 KiB, the 32-wave cap allows 8: registers and LDS both leave occupancy at the cap.
//   Loads: 4 x 16 bytes (n % 4 == 0) or 8 x 4 bytes per lane are issued, unconditionally and from indices clamped into the chunk, before
//   the first key is counted (docs/LAB_r17.md: one load at a time costs an L2 round trip per element).
//   Contention: a wave whose counted lanes all hold one bin (an all-equal or saturated sample: the worst case for 64 lanes on one LDS
//   word) adds its lane count once, from one lane.  Passes 1 and 2 count only the elements under the prefix, usually a few per cent.
//   Workspace per row (uint32 words): [0, 2048) pass 0 | [2048, 4096) pass 1, selections A and B | [4096, 6144) pass 2, A and B |
//   [6144, 6160) state: word 0 = number of NaNs, words 4 p .. 4 p + 3 = (prefix A, prefix B, remaining rank A, remaining rank B) entering
//   pass p = 1, 2.  Zeroed by the entry point on the stream, by a kernel of its own (abs_zero_kernel), and every pass has its own
//   histogram.  Not hipMemsetAsync: captured, its memset node zeroed the 98 560 bytes of a (4, 3072) workspace on the first replay of a
//   graph and filled them with a 16-byte pattern of two addresses on every later one (docs/LAB_r19.md) -- a kernel node replays as launched.
#include "pd_step.h"

namespace pd {

constexpr int AQ_THREADS = 256, AQ_CHUNK = PD_ABS_QUANTILE_CHUNK;
constexpr int AQ_HIST0 = 0, AQ_HIST1 = 2048, AQ_HIST2 = 4096, AQ_STATE = 6144, AQ_ROW_WORDS = 6160;
constexpr uint32_t AQ_INF = 0x7f800000u;
static_assert(AQ_CHUNK % (AQ_THREADS * 16) == 0, "a chunk is whole rounds of 16 elements per lane");

__device__ __forceinline__ int aq_hist_offset(int pass) { return pass == 0 ? AQ_HIST0 : (pass == 1 ? AQ_HIST1 : AQ_HIST2); }

// the workspace's words <- 0 (grid-stride)
__global__ __launch_bounds__(AQ_THREADS) void abs_zero_kernel(uint32_t* __restrict__ ws, const size_t words) {
  for (size_t i = (size_t)blockIdx.x * AQ_THREADS + threadIdx.x; i < words; i += (size_t)gridDim.x * AQ_THREADS) ws[i] = 0u;
}

// one key of every lane into histogram `h`: lanes with `in` count bin `digit`
__device__ __forceinline__ void aq_count(uint32_t* h, unsigned digit, bool in, int lane) {
  const unsigned long long act = __ballot(in);
  if (act == 0ull) return;
  const int leader = __ffsll((long long)act) - 1;
  const unsigned d0 = (unsigned)__shfl((int)digit, leader);
  const unsigned long long same = __ballot(in && digit == d0);
  if (same == act) {
    if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(act));
  } else if (in) {
    atomicAdd(&h[digit], 1u);
  }
}

// grid (chunks, B).  PASS 0 counts key >> 20 of every element (and the NaNs); PASS 1 / 2 count the next 10 bits of the elements whose
// higher bits equal a selection's prefix.  VEC: rows are 16-byte aligned (n % 4 == 0).
template <int PASS, bool VEC>
__global__ __launch_bounds__(AQ_THREADS) void abs_hist_kernel(const float* __restrict__ x, uint32_t* __restrict__ ws, const unsigned n) {
  constexpr int E = VEC ? 4 : 1, U = VEC ? 4 : 8, SHIFT = PASS == 0 ? 20 : (PASS == 1 ? 10 : 0);
  __shared__ uint32_t h[2048];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < 2048; i += AQ_THREADS) h[i] = 0u;
  uint32_t* const row = ws + (size_t)blockIdx.y * AQ_ROW_WORDS;
  unsigned preA = 0u, preB = 0u;
  if (PASS > 0) { preA = row[AQ_STATE + 4 * PASS]; preB = row[AQ_STATE + 4 * PASS + 1]; }
  const bool two = PASS > 0 && preA != preB;                            // (uniform over the workgroup)
  __syncthreads();
  const float* const xr = x + (size_t)blockIdx.y * n;
  const unsigned p0 = blockIdx.x * (unsigned)AQ_CHUNK;                  // < n < 2^31
  const unsigned cnt = n - p0 < (unsigned)AQ_CHUNK ? n - p0 : (unsigned)AQ_CHUNK;      // >= 1 (VEC: a multiple of 4, >= 4)
  unsigned nans = 0u;
  for (unsigned off = 0; off < cnt; off += AQ_THREADS * U * E) {        // (uniform trip count: the ballots see whole waves)
    uint32_t k[U * E];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned i = off + ((unsigned)u * AQ_THREADS + tid) * E;
      const unsigned ic = i < cnt ? i : cnt - E;
      if (VEC) {
        const uint4 v = *(const uint4*)(xr + p0 + ic);
        k[4 * u] = v.x; k[4 * u + 1] = v.y; k[4 * u + 2] = v.z; k[4 * u + 3] = v.w;
      } else {
        k[u] = __float_as_uint(xr[p0 + ic]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = off + ((unsigned)u * AQ_THREADS + tid) * E < cnt;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const uint32_t key = k[u * E + e] & 0x7fffffffu;                // |v|; -0 -> +0
        if (PASS == 0) {
          nans += (unsigned)__popcll(__ballot(valid && key > AQ_INF));
          aq_count(h, key >> 20, valid, lane);
        } else {
          const unsigned top = key >> (SHIFT + 10), digit = (key >> SHIFT) & 1023u;
          aq_count(h, digit, valid && top == preA, lane);
          if (two) aq_count(h + 1024, digit, valid && top == preB, lane);
        }
      }
    }
  }
  if (PASS == 0 && nans != 0u && lane == 0) atomicAdd(row + AQ_STATE, nans);
  __syncthreads();
  uint32_t* const out = row + aq_hist_offset(PASS);
  const int bins = (PASS == 0 || two) ? 2048 : 1024;
  for (int d = tid; d < bins; d += AQ_THREADS) {
    const uint32_t c = h[d];
    if (c) atomicAdd(out + d, c);
  }
}

// grid (B): the bin of pass PASS that holds each selection's remaining rank -> the state entering the next pass, or (PASS 2) the result
template <int PASS>
__global__ __launch_bounds__(AQ_THREADS) void abs_select_kernel(uint32_t* __restrict__ ws, float* __restrict__ out, const unsigned rank_lo,
                                                               const unsigned rank_hi, const float weight) {
#pragma clang fp contract(off)
  constexpr int NB = PASS == 0 ? 2048 : 1024, PER = NB / AQ_THREADS, BITS = PASS == 0 ? 11 : 10;
  __shared__ uint32_t part[AQ_THREADS];
  __shared__ uint32_t res[4];                                           // bin A, bin B, remaining rank A, remaining rank B
  const int tid = threadIdx.x;
  uint32_t* const row = ws + (size_t)blockIdx.x * AQ_ROW_WORDS;
  unsigned pre[2] = {0u, 0u}, rem[2] = {rank_lo, rank_hi};
  if (PASS > 0) {
    const uint32_t* const s = row + AQ_STATE + 4 * PASS;
    pre[0] = s[0]; pre[1] = s[1]; rem[0] = s[2]; rem[1] = s[3];
  }
  const bool two = PASS > 0 && pre[0] != pre[1];
  if (tid < 4) res[tid] = 0u;
#pragma unroll
  for (int sel = 0; sel < 2; ++sel) {
    const uint32_t* const hist = row + aq_hist_offset(PASS) + ((two && sel) ? 1024 : 0);
    uint32_t c[PER], sum = 0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) { c[j] = hist[tid * PER + j]; sum += c[j]; }
    __syncthreads();                                                    // (res cleared; the previous selection is done with part)
    part[tid] = sum;
    __syncthreads();
    uint32_t base = 0u;
    for (int j = 0; j < tid; ++j) base += part[j];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (rem[sel] >= base && rem[sel] - base < c[j]) { res[sel] = (uint32_t)(tid * PER + j); res[2 + sel] = rem[sel] - base; }
      base += c[j];
    }
  }
  __syncthreads();
  if (tid != 0) return;
  const uint32_t keyA = (pre[0] << BITS) | res[0], keyB = (pre[1] << BITS) | res[1];
  if (PASS < 2) {
    uint32_t* const s = row + AQ_STATE + 4 * (PASS + 1);
    s[0] = keyA; s[1] = keyB; s[2] = res[2]; s[3] = res[3];
  } else {
    const float a = __uint_as_float(keyA), b = __uint_as_float(keyB), d = b - a;
    const float v = weight < 0.5f ? a + weight * d : b - d * (1.0f - weight);
    out[blockIdx.x] = row[AQ_STATE] != 0u ? __uint_as_float(0x7fc00000u) : v;
  }
}

// ---- the step ------------------------------------------------------------------------------------------------------------------------------
// RAW: x0 -> `raw` only.  Otherwise the thresholded update.  Both take their operands from step_operands and their x0 from ddim_x0_eps
// (pd_step.h), so that they cannot differ.
template <bool RAW>
__global__ __launch_bounds__(256) void threshold_step_kernel(const pd_ddim_step_threshold_args a, float* __restrict__ raw) {
#pragma clang fp contract(off)
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= a.numel) return;
  const StepOperands r = step_operands(a, i0);
  float xp[4], x0v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float x0, eps;
    ddim_x0_eps(a, r.x[j], r.out[j], x0, eps);
    if (!RAW) {
      x0 = threshold_limit(x0, a.quantile[r.row[j]], a.sample_max_value);
      xp[j] = ddim_prev(a, r.x[j], x0, eps);
    }
    x0v[j] = x0;
  }
  if (!RAW) store_quad(a.prev_sample, i0, r.cnt, xp);
  float* const o0 = RAW ? raw : a.pred_x0;
  if (o0) store_quad(o0, i0, r.cnt, x0v);
}

// what both step entry points refuse; `x0`: pd_ddim_raw_x0's output (then prev_sample / pred_x0 / quantile are not looked at)
static int threshold_step_validate(const pd_ddim_step_threshold_args* a, const float* x0, bool raw, const char* who) {
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  if (const int rc = step_validate_common(a->numel, a->per_sample, a->pred_type, who, PD_ERR_SHAPE)) return rc;
  PD_CHECK(a->numel < (1ll << 41), PD_ERR_SHAPE, "%s: numel %lld overflows the grid (must be below 2^41)", who, (long long)a->numel);
  PD_CHECK(a->sample && a->model_out, PD_ERR_ARG, "%s: sample / model_out is NULL", who);
  PD_CHECK(!a->uncond_out || a->w, PD_ERR_ARG, "%s: guidance without weights", who);
  PD_CHECK((uintptr_t)a->w % 4 == 0, PD_ERR_ARG, "%s: w must be 4-byte aligned", who);
  if (raw) {
    PD_CHECK(x0 != nullptr, PD_ERR_ARG, "%s: x0 is NULL", who);
    return step_check_aligned16({{"sample", a->sample}, {"model_out", a->model_out}, {"uncond_out", a->uncond_out}, {"x0", x0}}, who);
  }
  PD_CHECK(a->prev_sample != nullptr, PD_ERR_ARG, "%s: prev_sample is NULL", who);
  PD_CHECK(a->quantile != nullptr, PD_ERR_ARG, "%s: quantile is NULL", who);
  PD_CHECK((uintptr_t)a->quantile % 4 == 0, PD_ERR_ARG, "%s: quantile must be 4-byte aligned", who);
  PD_CHECK(a->sample_max_value > 0.0f, PD_ERR_ARG, "%s: sample_max_value = %g (must be positive)", who, (double)a->sample_max_value);
  return step_check_aligned16({{"sample", a->sample}, {"model_out", a->model_out}, {"uncond_out", a->uncond_out},
                               {"prev_sample", a->prev_sample}, {"pred_x0", a->pred_x0}}, who);
}

static int abs_quantile_validate_sizes(int64_t B, int64_t n) {
  const char* const name = "pd_abs_quantile";
  PD_CHECK(B >= 1 && n >= 1, PD_ERR_SHAPE, "%s: B = %lld, n = %lld (both must be >= 1)", name, (long long)B, (long long)n);
  PD_CHECK(n < (1ll << 31), PD_ERR_SHAPE, "%s: n = %lld overflows the 32-bit counters (must be below 2^31)", name, (long long)n);
  PD_CHECK(B <= 65535, PD_ERR_SHAPE, "%s: B = %lld overflows the grid's second dimension (at most 65535 rows)", name, (long long)B);
  return PD_OK;
}

template <int PASS>
static void abs_quantile_pass(const pd_abs_quantile_args* a, hipStream_t st) {
  const dim3 grid((unsigned)((a->n + AQ_CHUNK - 1) / AQ_CHUNK), (unsigned)a->B);
  uint32_t* const ws = (uint32_t*)a->workspace;
  if (a->n % 4 == 0) hipLaunchKernelGGL((abs_hist_kernel<PASS, true>), grid, dim3(AQ_THREADS), 0, st, a->x, ws, (unsigned)a->n);
  else hipLaunchKernelGGL((abs_hist_kernel<PASS, false>), grid, dim3(AQ_THREADS), 0, st, a->x, ws, (unsigned)a->n);
  hipLaunchKernelGGL(abs_select_kernel<PASS>, dim3((unsigned)a->B), dim3(AQ_THREADS), 0, st, ws, a->out, (unsigned)a->rank_lo,
                     (unsigned)a->rank_hi, a->weight);
}

}  // namespace pd

using namespace pd;

extern "C" size_t pd_abs_quantile_workspace(int64_t B, int64_t n) {
  if (abs_quantile_validate_sizes(B, n) != PD_OK) return 0;
  return (size_t)B * AQ_ROW_WORDS * sizeof(uint32_t);
}

extern "C" int pd_abs_quantile(const pd_abs_quantile_args* a, void* stream) {
  const char* const name = "pd_abs_quantile";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", name);
  PD_CHECK(a->x && a->out && a->workspace, PD_ERR_ARG, "%s: null pointer (x, out, workspace)", name);
  const int rc = abs_quantile_validate_sizes(a->B, a->n);
  if (rc != PD_OK) return rc;
  PD_CHECK(a->rank_lo >= 0 && a->rank_lo <= a->rank_hi && a->rank_hi <= a->n - 1 && a->rank_hi - a->rank_lo <= 1, PD_ERR_ARG,
           "%s: rank_lo = %lld, rank_hi = %lld (0 <= rank_lo <= rank_hi <= n - 1 = %lld, at most 1 apart)", name, (long long)a->rank_lo,
           (long long)a->rank_hi, (long long)(a->n - 1));
  PD_CHECK(a->weight >= 0.0f && a->weight < 1.0f, PD_ERR_ARG, "%s: weight = %g (must be in [0, 1))", name, (double)a->weight);
  PD_CHECK((uintptr_t)a->x % (a->n % 4 == 0 ? 16 : 4) == 0, PD_ERR_ARG, "%s: x must be %d-byte aligned (n %% 4 %s 0)", name,
           a->n % 4 == 0 ? 16 : 4, a->n % 4 == 0 ? "==" : "!=");
  PD_CHECK((uintptr_t)a->out % 4 == 0 && (uintptr_t)a->workspace % 4 == 0, PD_ERR_ARG, "%s: out / workspace must be 4-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  const size_t words = (size_t)a->B * AQ_ROW_WORDS;
  const size_t blocks = (words + AQ_THREADS - 1) / AQ_THREADS;
  hipLaunchKernelGGL(abs_zero_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(AQ_THREADS), 0, st, (uint32_t*)a->workspace, words);
  PD_LAUNCH_CHECK();
  abs_quantile_pass<0>(a, st);
  PD_LAUNCH_CHECK();
  abs_quantile_pass<1>(a, st);
  PD_LAUNCH_CHECK();
  abs_quantile_pass<2>(a, st);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_ddim_raw_x0(const pd_ddim_step_threshold_args* a, float* x0, void* stream) {
  const int rc = threshold_step_validate(a, x0, true, "pd_ddim_raw_x0");
  if (rc != PD_OK) return rc;
  hipLaunchKernelGGL(threshold_step_kernel<true>, dim3((unsigned)((a->numel + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, *a, x0);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_ddim_step_threshold(const pd_ddim_step_threshold_args* a, void* stream) {
  const int rc = threshold_step_validate(a, nullptr, false, "pd_ddim_step_threshold");
  if (rc != PD_OK) return rc;
  hipLaunchKernelGGL(threshold_step_kernel<false>, dim3((unsigned)((a->numel + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, *a,
                     (float*)nullptr);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
