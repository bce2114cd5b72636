// Mask refinement: disc morphology through an exact Euclidean distance transform, connected components, hole filling and removal of
// small components -- the clean-up of a per-pixel contrast mask (mask_kernels.hip).  Contract: include/phendiff_hip.h.  Host side:
// phendiff_amd.mask_ops (mask_distance, mask_dilate / erode / open / close, mask_components, remove_small_components, fill_holes,
// MaskRefine, refine_mask).  Masks are dense uint8 [B][H][W], nonzero = set; H, W <= PD_MASK_MAX_SIDE.
//     pd_mask_distance    d2 = squared Euclidean distance to the nearest set (clear) pixel of the same sample, int32     2 launches
//     pd_mask_morph       DILATE: d2 to set <= r2;  ERODE: d2 to clear > r2                                               2 launches
//     pd_mask_components  label / area / border / count of one phase under 4- or 8-connectivity                           4 launches
//     pd_mask_filter      DROP_SMALL / FILL_HOLES from area and border, and the stats row                                 2 launches
//
// ATOMICS.  The house rule "no atomics" (pd_step.h, mask_kernels.hip) exists so that floating-point sums have one order.  Everything
// here is an integer, and integer atomicMin / atomicAdd / atomicOr give the same result in every order, so they are used: atomicMin on
// the union-find's parents, atomicAdd / atomicOr for a component's area and border flag at its root and for the counts of the stats
// rows.  Floating-point atomics are not allowed here either.
//
// The other house rules hold: a sample's result is a function of that sample alone (every index is formed within the sample: a pixel
// at a row's end is no neighbour of the next row's first pixel, a sample's last row none of the next sample's first); everything is
// validated before the first launch; no host read, no allocation: capturable.
//
// TERMINATION of the device loops is argued next to each of them; each also carries a hard cap it can never meet while parent[] holds
// what this file writes there, and sets the sample's status word instead of spinning if it does.
#include "pd_reduce.h"      // wave_reduce

namespace pd {
namespace {

constexpr int FAR = PD_MASK_FAR, MAX_SIDE = PD_MASK_MAX_SIDE;
constexpr int64_t MAX_BLOCKS = 65536;      // more items than this many blocks take are walked in a grid-stride loop
constexpr int AREA_BITS = 0x3fffffff, BORDER_BIT = 1 << 30;      // an area is at most 2^28: bit 30 of the root's word is the border flag
constexpr int FILTER_CHUNK = 1024;

static_assert((int64_t)MAX_SIDE * MAX_SIDE <= (1 << 28), "a sample's pixel index and area fit 28 bits");
static_assert(2 * (int64_t)MAX_SIDE * MAX_SIDE <= (int64_t)FAR, "H^2 + W^2 stays below PD_MASK_FAR");

unsigned grid_of(int64_t items, int per_block) {
  const int64_t blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

// ---- the distance transform ----------------------------------------------------------------------------------------------------------
struct DistLaunch {
  int64_t B;
  int H, W;
  const uint8_t* mask;
  int want;                      // 1: distance to set pixels, 0: to clear pixels
  int limit;                     // 0: none
  int32_t* g2;                   // [B][H][W]: written by the column pass, read by the row pass
  int32_t* d2;                   // row pass, distance form: may be g2 (a row is staged before it is rewritten); or NULL
  uint8_t* out;                  // row pass, morph form: the thresholded mask; or NULL
  int erode;                     // morph form: out = d2 > limit (else d2 <= limit)
  int32_t* stats;                // morph form: optional rows of PD_MASK_STATS_FIELDS words
  int64_t stats_stride;
  int stats_mode;                // PD_MORPH_STATS_IN: zero the row (column pass), count mask; PD_MORPH_STATS_OUT: count out
};

// Column pass: one thread per (sample, column); consecutive threads take consecutive columns, so every row's access is coalesced.  Down:
// the squared distance to the nearest wanted pixel at or above; up: the minimum with the nearest at or below.  Two loops of exactly H steps.
__global__ __launch_bounds__(256) void mask_column_kernel(const DistLaunch p) {
  const int64_t cols = p.B * p.W, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cols; i += stride) {
    const int64_t s = i / p.W;
    const int x = (int)(i - s * p.W);
    const uint8_t* m = p.mask + s * p.H * p.W + x;
    int32_t* g = p.g2 + s * p.H * p.W + x;
    if (x == 0 && p.stats && (p.stats_mode & PD_MORPH_STATS_IN)) {      // the sample's stats row: zeroed here, summed by the row passes
#pragma unroll
      for (int k = 0; k < PD_MASK_STATS_FIELDS; ++k) p.stats[s * p.stats_stride + k] = 0;
    }
    int last = -1;
    for (int y = 0; y < p.H; ++y) {
      if ((m[(int64_t)y * p.W] != 0) == (p.want != 0)) last = y;
      g[(int64_t)y * p.W] = last < 0 ? FAR : (y - last) * (y - last);
    }
    int next = -1;
    for (int y = p.H - 1; y >= 0; --y) {
      if ((m[(int64_t)y * p.W] != 0) == (p.want != 0)) next = y;
      if (next >= 0) {
        const int d = (next - y) * (next - y);
        if (d < g[(int64_t)y * p.W]) g[(int64_t)y * p.W] = d;
      }
    }
  }
}

// Row pass: a workgroup takes a (sample, row), stages the row's squared vertical distances in LDS (4 W bytes <= 64 KiB) and every thread
// walks outwards from its pixel: best = min over dx of dx^2 + g2[x +- dx].  The walk ends where dx^2 reaches the best so far (no farther
// column can win) or exceeds limit, and at dx = W - 1 at the latest: at most W steps.  g2 + dx^2 <= 2^30 + 2^28 fits an int32.
__global__ __launch_bounds__(256) void mask_row_kernel(const DistLaunch p) {
  extern __shared__ int32_t row[];
  const int t = threadIdx.x, lane = t & 63;      // (no static LDS: the staged row alone may take all 64 KiB)
  const int64_t rows = p.B * p.H;
  for (int64_t item = blockIdx.x; item < rows; item += gridDim.x) {
    const int64_t base = item * p.W, s = item / p.H;
    for (int x = t; x < p.W; x += 256) row[x] = p.g2[base + x];
    __syncthreads();
    int n_in = 0, n_out = 0;
    for (int x = t; x < p.W; x += 256) {
      int best = row[x];
      for (int d = 1; d < p.W; ++d) {
        const int dd = d * d;
        if (dd >= best || (p.limit > 0 && dd > p.limit)) break;
        if (x - d >= 0) { const int c = row[x - d] + dd; best = c < best ? c : best; }
        if (x + d < p.W) { const int c = row[x + d] + dd; best = c < best ? c : best; }
      }
      if (p.limit > 0 && best > p.limit) best = p.limit + 1;
      if (p.d2) p.d2[base + x] = best;
      if (p.out) {
        const int o = p.erode ? (best > p.limit) : (best <= p.limit);
        p.out[base + x] = (uint8_t)o;
        n_out += o;
        n_in += p.mask[base + x] != 0;
      }
    }
    if (p.stats && p.stats_mode) {      // (uniform) the row's two counts: wave butterfly, then one integer atomicAdd per wave and count
      n_in = wave_reduce<Sum>(n_in);
      n_out = wave_reduce<Sum>(n_out);
      if (lane == 0) {
        if ((p.stats_mode & PD_MORPH_STATS_IN) && n_in) atomicAdd(p.stats + s * p.stats_stride + PD_MS_PIXELS_IN, n_in);
        if ((p.stats_mode & PD_MORPH_STATS_OUT) && n_out) atomicAdd(p.stats + s * p.stats_stride + PD_MS_PIXELS_OUT, n_out);
      }
    }
    __syncthreads();      // (row is written again by the next item of a grid-stride walk)
  }
}

int launch_distance(const DistLaunch& p, hipStream_t stream) {
  hipLaunchKernelGGL(mask_column_kernel, dim3(grid_of(p.B * p.W, 256)), dim3(256), 0, stream, p);
  PD_LAUNCH_CHECK();
  const int64_t rows = p.B * p.H;
  hipLaunchKernelGGL(mask_row_kernel, dim3((unsigned)(rows < MAX_BLOCKS ? rows : MAX_BLOCKS)), dim3(256), (size_t)p.W * sizeof(int32_t), stream, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

// ---- connected components ------------------------------------------------------------------------------------------------------------
struct CompLaunch {
  pd_mask_components_args a;
  int hw;           // H * W <= 2^28
  int* parent;      // [B][hw]: within-sample indices; parent[i] <= i, and only ever lowered
  int* acc;         // [B][hw]: at a root, the component's area (low bits) and BORDER_BIT
};

__device__ __forceinline__ int load_relaxed(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of i's tree.  Every hop goes to a STRICTLY SMALLER index (parent[n] <= n always: init writes n, atomicMin only lowers) and the
// walk ends at the first fixed point, so it takes at most i + 1 <= hw iterations -- the cap, which is therefore never met.  On the way a
// node is pointed at its grandparent (ECL-CC's pointer jumping) with atomicMin: the grandparent is an ancestor, so no equivalence is
// lost, and parents stay monotone.  parent[] is read with relaxed atomic loads: other threads' atomicMin race with them, and the
// compiler may not keep a value across iterations.
__device__ int find_root(int* parent, int i, int cap, int* status, bool compress) {
  int n = i;
  for (int it = 0; it < cap; ++it) {
    const int p = load_relaxed(parent + n);
    if (p == n) return n;
    if (compress) {
      const int g = load_relaxed(parent + p);
      if (g < p) atomicMin(parent + n, g);
    }
    n = p;
  }
  if (status) atomicOr(status, 1);
  return n;
}

// Union of the trees of a and b: link the larger root under the smaller with atomicMin.  Where the atomicMin finds that the root was
// lowered in between (old != a: another thread linked it first), what this thread displaced or failed to record is the pair (old, b),
// and the loop goes on with it.  RETRIES: after a retry both indices are smaller than the larger root before it (old < a, b < a), so
// the larger of the two strictly decreases; it is at least 1 while they differ: at most hw - 1 retries, below the cap.
__device__ void unite(int* parent, int a, int b, int cap, int* status) {
  for (int it = 0; it < cap; ++it) {
    a = find_root(parent, a, cap, status, true);
    b = find_root(parent, b, cap, status, true);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }      // a: the larger root
    const int old = atomicMin(parent + a, b);
    if (old == a) return;                               // a was still a root: linked
    a = old;                                            // (old < a)
  }
  if (status) atomicOr(status, 2);
}

__global__ __launch_bounds__(256) void comp_init_kernel(const CompLaunch p) {
  const int64_t numel = p.a.B * p.hw, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const int64_t s = i / p.hw;
    const int j = (int)(i - s * p.hw);
    p.parent[i] = j;
    p.acc[i] = 0;
    if (j == 0) {
      if (p.a.count) p.a.count[s] = 0;
      if (p.a.status) p.a.status[s] = 0;
    }
  }
}

__global__ __launch_bounds__(256) void comp_merge_kernel(const CompLaunch p) {
  const int64_t numel = p.a.B * p.hw, stride = (int64_t)gridDim.x * 256;
  const int W = p.a.W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const int64_t s = i / p.hw;
    const int j = (int)(i - s * p.hw), y = j / W, x = j - y * W;
    const uint8_t* m = p.a.mask + s * p.hw;      // every neighbour is addressed WITHIN the sample, by (y, x)
    if ((m[j] != 0) != (p.a.phase != 0)) continue;
    int* parent = p.parent + s * p.hw;
    int* status = p.a.status ? p.a.status + s : nullptr;
    const bool want = p.a.phase != 0, eight = p.a.connectivity == 8;
    if (x > 0 && (m[j - 1] != 0) == want) unite(parent, j, j - 1, p.hw, status);
    if (y > 0) {
      if ((m[j - W] != 0) == want) unite(parent, j, j - W, p.hw, status);
      if (eight && x > 0 && (m[j - W - 1] != 0) == want) unite(parent, j, j - W - 1, p.hw, status);
      if (eight && x < W - 1 && (m[j - W + 1] != 0) == want) unite(parent, j, j - W + 1, p.hw, status);
    }
  }
}

// parent[i] = root(i); at the root the component's area and border flag.  The merges are complete (a kernel boundary lies between), so
// find_root gives the final root whatever other threads have flattened already.  A wave whose 64 pixels all have one root adds once.
// The loop's trip count is uniform over a wave (the bound is rounded up to whole waves): the wave-wide votes see every lane.
__global__ __launch_bounds__(256) void comp_flatten_kernel(const CompLaunch p) {
  const int64_t numel = p.a.B * p.hw, stride = (int64_t)gridDim.x * 256, padded = (numel + 63) / 64 * 64;
  const int W = p.a.W, H = p.a.H;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < padded; i += stride) {
    int64_t key = -1;      // the root's index in the whole batch; -1: no pixel, or the other phase
    int onb = 0;
    if (i < numel) {
      const int64_t s = i / p.hw;
      const int j = (int)(i - s * p.hw);
      if ((p.a.mask[i] != 0) == (p.a.phase != 0)) {
        int* parent = p.parent + s * p.hw;
        const int r = find_root(parent, j, p.hw, p.a.status ? p.a.status + s : nullptr, false);
        __hip_atomic_store(parent + j, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int y = j / W, x = j - y * W;
        onb = (y == 0 || y == H - 1 || x == 0 || x == W - 1) ? 1 : 0;
        key = s * p.hw + r;
        if (r == j && p.a.count) atomicAdd(p.a.count + s, 1);
      }
    }
    const int64_t k0 = __shfl(key, 0);
    if (__all(key == k0)) {
      const int any = __any(onb);
      if (k0 >= 0 && (threadIdx.x & 63) == 0) {
        atomicAdd(p.acc + k0, 64);
        if (any) atomicOr(p.acc + k0, BORDER_BIT);
      }
    } else if (key >= 0) {
      atomicAdd(p.acc + key, 1);
      if (onb) atomicOr(p.acc + key, BORDER_BIT);
    }
  }
}

__global__ __launch_bounds__(256) void comp_broadcast_kernel(const CompLaunch p) {
  const int64_t numel = p.a.B * p.hw, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const int64_t s = i / p.hw;
    int label = 0, area = 0, border = 0;
    if ((p.a.mask[i] != 0) == (p.a.phase != 0)) {
      const int r = p.parent[i];
      const int v = p.acc[s * p.hw + r];
      label = r + 1;
      area = v & AREA_BITS;
      border = (v & BORDER_BIT) ? 1 : 0;
    }
    if (p.a.label) p.a.label[i] = label;
    if (p.a.area) p.a.area[i] = area;
    if (p.a.border) p.a.border[i] = (uint8_t)border;
  }
}

// ---- the two filters -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void filter_init_kernel(const pd_mask_filter_args a) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= a.B) return;
  int32_t* st = a.stats + s * a.stats_stride;
  st[PD_MS_PIXELS_IN] = st[PD_MS_PIXELS_OUT] = st[PD_MS_COMPONENTS] = st[PD_MS_SELECTED] = 0;
  st[PD_MS_STATUS] = a.status ? a.status[s] : 0;
}

// A workgroup takes a (sample, chunk of FILTER_CHUNK pixels): thread t the pixels t, t + 256, ... of the chunk.
__global__ __launch_bounds__(256) void filter_kernel(const pd_mask_filter_args a, const int64_t chunks) {
  __shared__ int red[4][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int hw = a.H * a.W;
  for (int64_t item = blockIdx.x; item < a.B * chunks; item += gridDim.x) {
    const int64_t s = item / chunks;
    const int j0 = (int)(item - s * chunks) * FILTER_CHUNK;
    int n[4] = {0, 0, 0, 0};      // pixels in, pixels out, components, selected
    for (int j = j0 + t; j < j0 + FILTER_CHUNK && j < hw; j += 256) {
      const int64_t i = s * hw + j;
      const bool set = a.mask[i] != 0;
      const int area = a.area[i];
      bool o, sel;
      if (a.rule == PD_FILTER_DROP_SMALL) {
        sel = set && area >= a.area_limit;
        o = sel;
      } else {
        sel = !set && a.border[i] == 0 && (a.area_limit < 0 || area <= a.area_limit);
        o = set || sel;
      }
      a.out[i] = (uint8_t)o;
      const bool root = a.label[i] == j + 1;
      n[0] += set; n[1] += o; n[2] += root; n[3] += root && sel;
    }
    if (a.stats) {      // (uniform)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        n[k] = wave_reduce<Sum>(n[k]);
        if (lane == 0) red[k][wave] = n[k];
      }
      __syncthreads();
      if (t < 4) {
        const int v = red[t][0] + red[t][1] + red[t][2] + red[t][3];
        if (v) atomicAdd(a.stats + s * a.stats_stride + t, v);
      }
      __syncthreads();      // (red is written again by the next item of a grid-stride walk)
    }
  }
}

int validate_bhw(int64_t B, int H, int W, const char* who) {
  PD_CHECK(B >= 1, PD_ERR_SHAPE, "%s: B = %lld (must be >= 1)", who, (long long)B);
  PD_CHECK(H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE, PD_ERR_SHAPE, "%s: H x W = %d x %d (each side 1 to %d)", who, H, W, MAX_SIDE);
  PD_CHECK(B < (1ll << 60) / ((int64_t)H * W), PD_ERR_SHAPE, "%s: B * H * W = %lld * %d * %d does not fit 60 bits", who, (long long)B, H, W);
  return PD_OK;
}

bool sizes_ok(int64_t B, int H, int W) {
  return B >= 1 && H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE && B < (1ll << 60) / ((int64_t)H * W);
}

}  // namespace
}  // namespace pd

using namespace pd;

extern "C" int pd_mask_distance(const pd_mask_distance_args* a, void* stream) {
  const char* const who = "pd_mask_distance";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->mask != nullptr, PD_ERR_ARG, "%s: mask is NULL", who);
  PD_CHECK(a->d2 != nullptr, PD_ERR_ARG, "%s: d2 is NULL", who);
  PD_CHECK((uintptr_t)a->d2 % 4 == 0, PD_ERR_ARG, "%s: d2 must be 4-byte aligned", who);
  if (const int rc = validate_bhw(a->B, a->H, a->W, who)) return rc;
  PD_CHECK(a->limit >= 0 && a->limit < FAR, PD_ERR_SHAPE, "%s: limit = %d (0 for none, else below PD_MASK_FAR = %d)", who, a->limit, FAR);
  DistLaunch p = {};
  p.B = a->B; p.H = a->H; p.W = a->W;
  p.mask = a->mask; p.want = a->to_set != 0; p.limit = a->limit;
  p.g2 = a->d2; p.d2 = a->d2;
  return launch_distance(p, (hipStream_t)stream);
}

extern "C" size_t pd_mask_morph_workspace(int64_t B, int H, int W) {
  return sizes_ok(B, H, W) ? (size_t)(B * H * W) * sizeof(int32_t) : 0;
}

extern "C" int pd_mask_morph(const pd_mask_morph_args* a, void* stream) {
  const char* const who = "pd_mask_morph";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->mask != nullptr, PD_ERR_ARG, "%s: mask is NULL", who);
  PD_CHECK(a->out != nullptr, PD_ERR_ARG, "%s: out is NULL", who);
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "%s: null workspace (pd_mask_morph_workspace gives its size)", who);
  PD_CHECK((uintptr_t)a->workspace % 4 == 0, PD_ERR_ARG, "%s: workspace must be 4-byte aligned", who);
  PD_CHECK((uintptr_t)a->stats % 4 == 0, PD_ERR_ARG, "%s: stats must be 4-byte aligned", who);
  PD_CHECK(a->stats_mode >= 0 && a->stats_mode <= (PD_MORPH_STATS_IN | PD_MORPH_STATS_OUT), PD_ERR_ARG, "%s: stats_mode = %d (PD_MORPH_STATS_IN | PD_MORPH_STATS_OUT)",
           who, a->stats_mode);
  PD_CHECK(a->op == PD_MORPH_DILATE || a->op == PD_MORPH_ERODE, PD_ERR_ARG, "%s: op = %d (PD_MORPH_DILATE or PD_MORPH_ERODE)", who, a->op);
  if (const int rc = validate_bhw(a->B, a->H, a->W, who)) return rc;
  PD_CHECK(a->r2 >= 0 && a->r2 < FAR, PD_ERR_SHAPE, "%s: r2 = %d (0 to PD_MASK_FAR - 1 = %d)", who, a->r2, FAR - 1);
  PD_CHECK(!a->stats || a->stats_stride >= PD_MASK_STATS_FIELDS, PD_ERR_SHAPE, "%s: stats_stride = %lld (a row is %d words)", who, (long long)a->stats_stride,
           PD_MASK_STATS_FIELDS);
  const uintptr_t n = (uintptr_t)(a->B * a->H * a->W), m0 = (uintptr_t)a->mask, o0 = (uintptr_t)a->out;
  PD_CHECK(o0 + n <= m0 || m0 + n <= o0, PD_ERR_ARG, "%s: out may not alias mask (a pixel's result reads its whole neighbourhood)", who);
  DistLaunch p = {};
  p.B = a->B; p.H = a->H; p.W = a->W;
  p.mask = a->mask; p.want = a->op == PD_MORPH_DILATE; p.limit = a->r2;
  p.g2 = (int32_t*)a->workspace; p.out = a->out; p.erode = a->op == PD_MORPH_ERODE;
  p.stats = a->stats; p.stats_stride = a->stats_stride; p.stats_mode = a->stats_mode;
  return launch_distance(p, (hipStream_t)stream);
}

extern "C" size_t pd_mask_components_workspace(int64_t B, int H, int W) {
  return sizes_ok(B, H, W) ? (size_t)(B * H * W) * 2 * sizeof(int32_t) : 0;
}

extern "C" int pd_mask_components(const pd_mask_components_args* a, void* stream) {
  const char* const who = "pd_mask_components";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->mask != nullptr, PD_ERR_ARG, "%s: mask is NULL", who);
  PD_CHECK(a->workspace != nullptr, PD_ERR_ARG, "%s: null workspace (pd_mask_components_workspace gives its size)", who);
  PD_CHECK(a->label || a->area || a->border || a->count, PD_ERR_ARG, "%s: no output (label, area, border and count are all NULL)", who);
  PD_CHECK((uintptr_t)a->workspace % 4 == 0 && (uintptr_t)a->label % 4 == 0 && (uintptr_t)a->area % 4 == 0 && (uintptr_t)a->count % 4 == 0 &&
               (uintptr_t)a->status % 4 == 0,
           PD_ERR_ARG, "%s: workspace, label, area, count and status must be 4-byte aligned", who);
  if (const int rc = validate_bhw(a->B, a->H, a->W, who)) return rc;
  PD_CHECK(a->connectivity == 4 || a->connectivity == 8, PD_ERR_SHAPE, "%s: connectivity = %d (4 or 8)", who, a->connectivity);
  PD_CHECK(a->phase == 0 || a->phase == 1, PD_ERR_SHAPE, "%s: phase = %d (1: the set pixels, 0: the clear pixels)", who, a->phase);
  CompLaunch p;
  p.a = *a;
  p.hw = a->H * a->W;
  p.parent = (int*)a->workspace;
  p.acc = p.parent + a->B * p.hw;
  const int64_t numel = a->B * p.hw;
  const unsigned grid = grid_of(numel, 256);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(comp_init_kernel, dim3(grid), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(comp_merge_kernel, dim3(grid), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(comp_flatten_kernel, dim3(grid), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(comp_broadcast_kernel, dim3(grid), dim3(256), 0, st, p);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

extern "C" int pd_mask_filter(const pd_mask_filter_args* a, void* stream) {
  const char* const who = "pd_mask_filter";
  PD_CHECK(a != nullptr, PD_ERR_ARG, "%s: null args", who);
  PD_CHECK(a->mask != nullptr, PD_ERR_ARG, "%s: mask is NULL", who);
  PD_CHECK(a->label != nullptr && a->area != nullptr && a->border != nullptr, PD_ERR_ARG, "%s: label / area / border is NULL (pd_mask_components writes them)", who);
  PD_CHECK(a->out != nullptr, PD_ERR_ARG, "%s: out is NULL", who);
  PD_CHECK((uintptr_t)a->label % 4 == 0 && (uintptr_t)a->area % 4 == 0 && (uintptr_t)a->status % 4 == 0 && (uintptr_t)a->stats % 4 == 0, PD_ERR_ARG,
           "%s: label, area, status and stats must be 4-byte aligned", who);
  PD_CHECK(a->rule == PD_FILTER_DROP_SMALL || a->rule == PD_FILTER_FILL_HOLES, PD_ERR_ARG, "%s: rule = %d (PD_FILTER_DROP_SMALL or PD_FILTER_FILL_HOLES)", who,
           a->rule);
  if (const int rc = validate_bhw(a->B, a->H, a->W, who)) return rc;
  PD_CHECK(a->rule != PD_FILTER_DROP_SMALL || a->area_limit >= 0, PD_ERR_SHAPE, "%s: min_area = %d (must be >= 0)", who, a->area_limit);
  PD_CHECK(!a->stats || a->stats_stride >= PD_MASK_STATS_FIELDS, PD_ERR_SHAPE, "%s: stats_stride = %lld (a row is %d words)", who, (long long)a->stats_stride,
           PD_MASK_STATS_FIELDS);
  hipStream_t st = (hipStream_t)stream;
  if (a->stats) {
    hipLaunchKernelGGL(filter_init_kernel, dim3((unsigned)((a->B + 255) / 256)), dim3(256), 0, st, *a);
    PD_LAUNCH_CHECK();
  }
  const int64_t chunks = ((int64_t)a->H * a->W + FILTER_CHUNK - 1) / FILTER_CHUNK, items = a->B * chunks;
  hipLaunchKernelGGL(filter_kernel, dim3((unsigned)(items < MAX_BLOCKS ? items : MAX_BLOCKS)), dim3(256), 0, st, *a, chunks);
  PD_LAUNCH_CHECK();
  return PD_OK;
}
