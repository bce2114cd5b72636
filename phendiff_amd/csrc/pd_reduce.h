// The determinism rule of the per-sample statistics, once, as code.  Every reduction that promises a sample's bits runs in ONE order:
//   lane       a thread's own elements by ascending index (the kernel's loop; its start values and per-element expressions stay there)
//   wave       xor butterfly with masks 32, 16, ... 1: lane l combines its value with lane l ^ m's (wave_reduce)
//   workgroup  lane 0 of wave w puts red[w]; after one barrier the result is ((red[0] o red[1]) o red[2]) o red[3] (block_reduce)
//   chunks     thread r starts from record r * per ITSELF -- not from an identity combined with it: 0.0 + (-0.0) is +0.0 -- and combines
//              the following records of its run of `per` consecutive records in index order; thread 0 then starts from run 0 and combines
//              runs 1 .. runs - 1 in index order (run_fold), per = ceil(count / 256), runs = ceil(count / per)
// The order depends on sizes alone, so a sample's result does not depend on the batch, the row, the alignment, the grid or the replay.
// Users: pd_sample_stats, pd_guidance_rescale, pd_contrast_mask, pd_ssim, pd_object_intensity, pd_kid_mmd (all four levels or the first
// three); mask_morph.hip's integer counts (wave_reduce, then integer atomics, which have no order).
//
// There is no floating-point multiplication in this file: contraction cannot enter a sum through it, whatever the caller's pragma says.
#pragma once
#include <utility>

#include "pd_common.h"

namespace pd {

// ---- operations: an identity and apply(a, b), a the value held, b the one that arrives ----------------------------------------------------
// The two minimum / maximum flavours are NOT the same function: fmin / fmax pass over a NaN (it loses against any number), the
// compare-and-select forms never take one (a NaN held stays, a NaN that arrives is dropped).
struct Sum {      // double, int, long long
  template <typename T> static __device__ __forceinline__ T identity() { return T(0); }
  template <typename T> static __device__ __forceinline__ T apply(T a, T b) { return a + b; }
};
struct Or {       // int
  template <typename T> static __device__ __forceinline__ T identity() { return T(0); }
  template <typename T> static __device__ __forceinline__ T apply(T a, T b) { return a | b; }
};
struct Fmin {
  static __device__ __forceinline__ double identity() { return (double)INFINITY; }
  static __device__ __forceinline__ double apply(double a, double b) { return fmin(a, b); }
};
struct Fmax {
  static __device__ __forceinline__ double identity() { return -(double)INFINITY; }
  static __device__ __forceinline__ double apply(double a, double b) { return fmax(a, b); }
};
struct SelectMin {
  static __device__ __forceinline__ double identity() { return (double)INFINITY; }
  static __device__ __forceinline__ double apply(double a, double b) { return b < a ? b : a; }
};
struct SelectMax {
  static __device__ __forceinline__ double identity() { return -(double)INFINITY; }
  static __device__ __forceinline__ double apply(double a, double b) { return b > a ? b : a; }
};
template <typename... Op> struct Ops { static constexpr int N = sizeof...(Op); };      // value i of a record combines by the i-th of them

// ---- wave: every lane ends with the result ------------------------------------------------------------------------------------------------
template <typename Op, typename T> __device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = Op::apply(v, __shfl_xor(v, m));
  return v;
}

// ---- workgroup of 256 threads, N values at once -------------------------------------------------------------------------------------------
// The caller owns red ([4][N], __shared__: the LDS a kernel takes stays visible in the kernel) and, in a grid-stride loop, the barrier
// before red is written again.  block_put / block_get are block_reduce's two halves, for a kernel that reduces records of two types
// under one barrier.  Every thread ends with the result in v.
template <typename T, typename... Op, size_t... I>
__device__ __forceinline__ void block_put(T (&v)[sizeof...(Op)], T (*red)[sizeof...(Op)], std::index_sequence<I...>) {
  ((v[I] = wave_reduce<Op>(v[I])), ...);
  if ((threadIdx.x & 63) == 0) ((red[threadIdx.x >> 6][I] = v[I]), ...);
}
template <typename T, typename... Op, size_t... I>
__device__ __forceinline__ void block_get(T (&v)[sizeof...(Op)], T (*red)[sizeof...(Op)], std::index_sequence<I...>) {
  ((v[I] = Op::apply(Op::apply(Op::apply(red[0][I], red[1][I]), red[2][I]), red[3][I])), ...);
}
template <typename T, typename... Op> __device__ __forceinline__ void block_put(Ops<Op...>, T (&v)[sizeof...(Op)], T (*red)[sizeof...(Op)]) {
  block_put<T, Op...>(v, red, std::index_sequence_for<Op...>());
}
template <typename T, typename... Op> __device__ __forceinline__ void block_get(Ops<Op...>, T (&v)[sizeof...(Op)], T (*red)[sizeof...(Op)]) {
  block_get<T, Op...>(v, red, std::index_sequence_for<Op...>());
}
template <typename T, typename... Op> __device__ __forceinline__ void block_reduce(Ops<Op...> ops, T (&v)[sizeof...(Op)], T (*red)[sizeof...(Op)]) {
  block_put(ops, v, red);
  __syncthreads();
  block_get(ops, v, red);
}
template <typename Op, typename T> __device__ __forceinline__ T block_reduce(T v, T (&red)[4]) {      // one value
  T a[1] = {v};
  block_reduce(Ops<Op>(), a, reinterpret_cast<T(*)[1]>(red));
  return a[0];
}

// ---- chunks: `count` >= 1 records of N doubles at `in` -> r, in thread 0 ONLY ----------------------------------------------------------------
// red: [256][N], __shared__, the caller's, as is the barrier before it is written again.  One barrier inside; every thread must call.
template <typename... Op, size_t... I>
__device__ __forceinline__ void run_fold(const double* in, int64_t count, double (*red)[sizeof...(Op)], double (&r)[sizeof...(Op)],
                                         std::index_sequence<I...>) {
  constexpr int N = sizeof...(Op);
  const int64_t per = (count + 255) / 256;
  const int runs = (int)((count + per - 1) / per), t = threadIdx.x;      // <= 256 runs, every one of them non-empty
  if (t < runs) {
    const int64_t c0 = t * per, c1 = c0 + per < count ? c0 + per : count;
    double acc[N];
    ((acc[I] = in[c0 * N + I]), ...);
    for (int64_t c = c0 + 1; c < c1; ++c) ((acc[I] = Op::apply(acc[I], in[c * N + I])), ...);
    ((red[t][I] = acc[I]), ...);
  }
  __syncthreads();
  if (t == 0) {
    ((r[I] = red[0][I]), ...);
    for (int u = 1; u < runs; ++u) ((r[I] = Op::apply(r[I], red[u][I])), ...);
  }
}
template <typename... Op>
__device__ __forceinline__ void run_fold(Ops<Op...>, const double* in, int64_t count, double (*red)[sizeof...(Op)], double (&r)[sizeof...(Op)]) {
  run_fold<Op...>(in, count, red, r, std::index_sequence_for<Op...>());
}

// ---- a sample of n elements cut into chunks of `chunk`, one workgroup per (sample, chunk) pair ----------------------------------------------
// chunks per sample, or 0 where the sizes are refused (the flat index, the workspace's size and the grid must fit).  An entry point's own
// lower bound on n, with its message, stays at the entry point.
static inline int64_t chunks_of(int64_t B, int64_t n, int chunk) {
  if (B < 1 || n < 1 || n >= (1ll << 62) / B) return 0;
  const int64_t chunks = (n + chunk - 1) / chunk;
  return chunks > ((1ll << 31) - 1) / B ? 0 : chunks;
}

// where pair `item` lies: the row, the chunk's first element within the row, its number of elements
struct ChunkTile { int64_t b, j0; int rem; };
__device__ __forceinline__ ChunkTile chunk_tile(int64_t item, int64_t chunks, int64_t n, int chunk) {
  ChunkTile t;
  t.b = item / chunks;
  t.j0 = (item - t.b * chunks) * chunk;
  const int64_t left = n - t.j0;
  t.rem = left < chunk ? (int)left : chunk;
  return t;
}

}  // namespace pd
