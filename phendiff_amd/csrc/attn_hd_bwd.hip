// pd_attn_hd_bwd: gradient of pd_attn_hd (softmax(q k^T * scale) v per (batch, head)), templated on the head dimension as the forward is and built
// for D = 16 / 32 (attention_head_dim 16 / 32 of the pixel UNet).  P is recomputed from the forward's log-sum-exp (log2 domain, scale included).
// The split of pd_attn_d64_bwd (sd_bwd_kernels.hip): every reduction is lane-local, there are no atomics, the result is bitwise reproducible.
//   delta pre-pass : delta[i] = sum_d o[i][d] * do[i][d], one thread per (row, head)
//   dQ kernel      : query on the lane.  Per 32-key sub-tile  S^T = K.Q^T,  dP^T = V.dO^T  (K / V rows from LDS, Q^T / dO^T fragments in registers),
//                    dS^T = P^T o (dP^T - delta)  lane-local,  dQ^T += K^T . dS^T  (transposed read of the same K tile)
//   dK/dV kernel   : key on the lane.  Per 32-query sub-tile  S = Q.K^T,  dP = dO.V^T  (Q / dO rows from LDS, K^T / V^T fragments in registers),
//                    dV^T += dO^T . P,  dK^T += Q^T . dS  (transposed reads of the dO / Q tiles)
// Padding as the forward's (pd_hd.h): a contraction over d takes DK / 16 k-steps, a result with d as its row takes DV / 32 row tiles.  Every LDS tile
// here is [rows][DV] at the transposed-read pitch, because it is read both ways; its pad columns D .. DV are zeroed once per workgroup (the staging
// writes columns < D only) and the pad pieces of the register fragments are selected to zero.  Nothing is read from HBM for a pad channel (the
// channels behind a head belong to the next head, or to nobody) and no pad channel of dq / dk / dv is stored.
// Rows >= Nkv / >= Nq: their staging offsets are SELECTED to OOB_OFF (zeros, whatever the range check of the buffer instruction covers: DESIGN.md,
// "Buffer-resource bounds"), their P / dS entries are selected to zero and their rows are not stored.
// The scale is applied to the fp32 scores, not to a 16-bit q or k (attn_hd.hip: a second rounding of q is the error of P with few keys); dq and dk
// take it once more at the store.
#include <stdlib.h>
#include "pd_common.h"
#include "pd_stage.h"
#include "pd_hd.h"

namespace pd {

// LDS tile of the backward kernels: [RT rows][DV] at pitch HD::VP, read as row fragments (contraction over d) and as transposed blocks
template <typename T, int D> struct HDB {
  typedef HD<T, D> X;
  typedef Elem<T> E;
  typedef typename E::Frag Frag;
  static constexpr int ES = X::ES, TP = X::VP, RT = X::KT;                 // rows per tile: the forward's keys per tile
  static constexpr int TB = RT * TP;                                       // bytes of one tile
  static constexpr int LDS_DQ = 2 * 2 * TB;                                // [2][K tile | V tile]
  static constexpr int BUF_DKV = 2 * TB + 2 * RT * 4;                      // Q tile | dO tile | lse[RT] | delta[RT]
  static constexpr int LDS_DKV = 2 * BUF_DKV;
  static_assert(TP >= X::DV * ES && TP % 16 == 0, "a tile row holds DV elements in 16-byte pieces");
  // zeros in the pad columns D .. DV of one tile row
  static __device__ __forceinline__ void zero_pad(unsigned char* row) {
#pragma unroll
    for (int o = D * ES; o < X::DV * ES; o += 16) *(u32x4*)(row + o) = (u32x4)(0u);
  }
  // fragment of 8 channels d0 .. d0 + 7 of a token row in HBM; a pad piece (d0 >= D) is zeros and reads nothing
  static __device__ __forceinline__ Frag load_piece(const T* row, int d0) {
    const bool real = d0 < D;                                              // (D is a multiple of 8: a piece is real or padding as a whole)
    Frag f = E::load(row + (real ? d0 : 0));
    if (!real) f = E::zero();
    return f;
  }
};

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_hd_delta_kernel(const pd_attn_hd_bwd_args a) {
  using E = Elem<T>;
  constexpr int PPR = HD<T, D>::PPR;
  const size_t total = (size_t)a.B * a.Nq * a.heads;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int head = (int)(idx % a.heads);
  const size_t row = idx / a.heads;                                        // b * Nq + i
  const T* op = (const T*)a.o + row * a.o_stride + head * D;
  const T* dp = (const T*)a.dout + row * a.o_stride + head * D;
  float s = 0.f;
#pragma unroll
  for (int pc = 0; pc < PPR; ++pc) {
    float o[8], d[8];
    E::unpack(E::load(op + pc * 8), o);
    E::unpack(E::load(dp + pc * 8), d);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += o[j] * d[j];
  }
  const size_t b = row / a.Nq, i = row - b * a.Nq;
  a.delta[(b * a.heads + head) * a.Nq + i] = s;
}

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_hd_dq_kernel(const pd_attn_hd_bwd_args a) {
  using E = Elem<T>;
  using Frag = typename E::Frag;
  using X = HD<T, D>;
  using XB = HDB<T, D>;
  constexpr int KT = XB::RT, TP = XB::TP, TB = XB::TB, ES = X::ES, KS = X::KS, NT = X::NT, PPR = X::PPR, PIECES = X::PIECES;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // [2][K tile | V tile]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nqb = (a.Nq + 127) / 128;
  const int item = xcd_chunk_index((int)blockIdx.x, nqb * a.heads * a.B);    // query blocks of one head stream the same K / V: one XCD / L2
  const int qb = item % nqb, head = (item / nqb) % a.heads, b = item / (nqb * a.heads);
  const T* qp = (const T*)a.q + (size_t)b * a.Nq * a.q_stride + head * D;
  const T* kp = (const T*)a.k + (size_t)b * a.Nkv * a.kv_stride + head * D;
  const T* vp = (const T*)a.v + (size_t)b * a.Nkv * a.kv_stride + head * D;
  const T* dop = (const T*)a.dout + (size_t)b * a.Nq * a.o_stride + head * D;

  if (tid < 2 * KT) {                                   // pad columns of both tiles of both buffers
    unsigned char* row = lds + (tid / KT) * 2 * TB + (tid % KT) * TP;
    XB::zero_pad(row);
    XB::zero_pad(row + TB);
  }

  // Q^T / dO^T fragments (B operands): lane (query r, h), k-step ks: d = 16 ks + 8 h + j; queries >= Nq re-read the last query and are not stored
  const int query = qb * 128 + wave * 32 + r, qc = min(query, a.Nq - 1);
  const float qscale = a.scale * 1.4426950408889634f;
  Frag qf[KS], dof[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = XB::load_piece(qp + (size_t)qc * a.q_stride, 16 * ks + 8 * h);
    dof[ks] = XB::load_piece(dop + (size_t)qc * a.o_stride, 16 * ks + 8 * h);
  }
  const size_t stat = ((size_t)b * a.heads + head) * a.Nq + qc;
  const float lse = a.lse[stat], delta = a.delta[stat];
  f32x16 dq[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dq[t] = (f32x16)(0.f);

  Frag stk[PIECES], stv[PIECES];
  const unsigned kv_bytes = (unsigned)(((size_t)(a.Nkv - 1) * a.kv_stride + D) * ES);      // this (batch, head)'s slice ends with its last key's D channels
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)kp, 0, kv_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)vp, 0, kv_bytes, 0x00020000);
  int prow[PIECES], psub[PIECES];
  unsigned kvoff[PIECES];
#pragma unroll
  for (int i = 0; i < PIECES; ++i) {
    const int pc = tid + 256 * i;
    prow[i] = pc / PPR; psub[i] = pc % PPR;
    kvoff[i] = ((unsigned)prow[i] * (unsigned)a.kv_stride + (unsigned)psub[i] * 8u) * (unsigned)ES;    // unsigned: a row past Nkv may wrap, and is selected away
    if (pc >= X::NP) prow[i] = 0x40000000;                              // no such piece: never in range, never committed
  }
  auto issue = [&](int k0) {
    const unsigned so = (unsigned)k0 * (unsigned)a.kv_stride * ES;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const unsigned off = (prow[i] < a.Nkv - k0) ? kvoff[i] + so : OOB_OFF;      // a key at or past Nkv: zeros, by selection
      stk[i] = E::load_buf(rk, off, 0);
      stv[i] = E::load_buf(rv, off, 0);
    }
  };
  auto commit = [&](int buf) {
    unsigned char* kb = lds + buf * 2 * TB;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      if (tid + 256 * i < X::NP) {
        const int off = prow[i] * TP + psub[i] * 8 * ES;
        E::store(kb + off, stk[i]);
        E::store(kb + TB + off, stv[i]);
      }
    }
  };
  const int row_lane = r * TP + 8 * h * ES;            // row fragment: row r, d = 16 ks + 8 h + (0..7)
  const int t_lane = X::vt_lane_off(lane);

  issue(0);
  commit(0);
  if (KT < a.Nkv) issue(KT);
  __syncthreads();
  for (int k0 = 0, cur = 0; k0 < a.Nkv; k0 += KT, cur ^= 1) {
    const unsigned char* kb = lds + cur * 2 * TB;
    const unsigned char* vb = kb + TB;
#pragma unroll
    for (int sub = 0; sub < KT / 32; ++sub) {
      if (k0 + sub * 32 < a.Nkv) {                     // workgroup-uniform
        f32x16 s = (f32x16)(0.f), dp = (f32x16)(0.f);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          s = E::mma(E::load(kb + row_lane + sub * 32 * TP + ks * 16 * ES), qf[ks], s);
          dp = E::mma(E::load(vb + row_lane + sub * 32 * TP + ks * 16 * ES), dof[ks], dp);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(s[i] * qscale - lse);
          s[i] = p * (dp[i] - delta);                    // dS^T
        }
        if (k0 + sub * 32 + 32 > a.Nkv) {               // keys beyond the context length (workgroup-uniform): dS = 0, by selection
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (k0 + sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * h >= a.Nkv) s[i] = 0.f;
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const Frag df = D64<T>::pack_p(s, st);
          const unsigned char* kt = kb + t_lane + (sub * 32 + 16 * st) * TP;
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) dq[tt] = E::mma(X::load_vt(kt + tt * 32 * ES), df, dq[tt]);
        }
      }
    }
    if (k0 + KT < a.Nkv) {
      commit(cur ^ 1);
      if (k0 + 2 * KT < a.Nkv) issue(k0 + 2 * KT);
    }
    __syncthreads();
  }
  if (query < a.Nq) {
    const float sc = a.scale;
    T* dst = (T*)a.dq + ((size_t)b * a.Nq + query) * a.dq_stride + head * D + 4 * h;
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
      for (int g = 0; g < 4; ++g)                        // register 4g + i <-> d = 32 tt + 8g + 4h + i; groups at d >= D are padding
        if (32 * tt + 8 * g < D)
          store4(dst + 32 * tt + 8 * g, dq[tt][4 * g] * sc, dq[tt][4 * g + 1] * sc, dq[tt][4 * g + 2] * sc, dq[tt][4 * g + 3] * sc);
  }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_hd_dkv_kernel(const pd_attn_hd_bwd_args a) {
  using E = Elem<T>;
  using Frag = typename E::Frag;
  using X = HD<T, D>;
  using XB = HDB<T, D>;
  constexpr int QT = XB::RT, TP = XB::TP, TB = XB::TB, BUF = XB::BUF_DKV, ES = X::ES, KS = X::KS, NT = X::NT, PPR = X::PPR, PIECES = X::PIECES;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // [2][Q tile | dO tile | lse | delta]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nkb = (a.Nkv + 127) / 128;
  const int item = xcd_chunk_index((int)blockIdx.x, nkb * a.heads * a.B);    // a head's key blocks share Q / dO
  const int kblk = item % nkb, head = (item / nkb) % a.heads, b = item / (nkb * a.heads);
  const T* qp = (const T*)a.q + (size_t)b * a.Nq * a.q_stride + head * D;
  const T* kp = (const T*)a.k + (size_t)b * a.Nkv * a.kv_stride + head * D;
  const T* vp = (const T*)a.v + (size_t)b * a.Nkv * a.kv_stride + head * D;
  const T* dop = (const T*)a.dout + (size_t)b * a.Nq * a.o_stride + head * D;
  const float* lsep = a.lse + ((size_t)b * a.heads + head) * a.Nq;
  const float* delp = a.delta + ((size_t)b * a.heads + head) * a.Nq;

  if (tid < 2 * QT) {                                   // pad columns of both tiles of both buffers
    unsigned char* row = lds + (tid / QT) * BUF + (tid % QT) * TP;
    XB::zero_pad(row);
    XB::zero_pad(row + TB);
  }

  // K^T / V^T fragments (B operands): lane (key r, h), k-step ks: d = 16 ks + 8 h + j; keys >= Nkv re-read the last key and are not stored
  // (their columns of S / dP feed only their own, unstored, dk / dv)
  const int key = kblk * 128 + wave * 32 + r, kc = min(key, a.Nkv - 1);
  const float kscale = a.scale * 1.4426950408889634f;
  Frag kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = XB::load_piece(kp + (size_t)kc * a.kv_stride, 16 * ks + 8 * h);
    vf[ks] = XB::load_piece(vp + (size_t)kc * a.kv_stride, 16 * ks + 8 * h);
  }
  f32x16 dk[NT], dv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { dk[t] = (f32x16)(0.f); dv[t] = (f32x16)(0.f); }

  Frag stq[PIECES], std_[PIECES];
  const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)qp, 0, (unsigned)(((size_t)(a.Nq - 1) * a.q_stride + D) * ES), 0x00020000);
  const __amdgpu_buffer_rsrc_t rdo = __builtin_amdgcn_make_buffer_rsrc((void*)dop, 0, (unsigned)(((size_t)(a.Nq - 1) * a.o_stride + D) * ES), 0x00020000);
  int prow[PIECES], psub[PIECES];
  unsigned qoff[PIECES], dooff[PIECES];
#pragma unroll
  for (int i = 0; i < PIECES; ++i) {
    const int pc = tid + 256 * i;
    prow[i] = pc / PPR; psub[i] = pc % PPR;
    qoff[i] = ((unsigned)prow[i] * (unsigned)a.q_stride + (unsigned)psub[i] * 8u) * (unsigned)ES;      // unsigned: a row past Nq may wrap, and is selected away
    dooff[i] = ((unsigned)prow[i] * (unsigned)a.o_stride + (unsigned)psub[i] * 8u) * (unsigned)ES;
    if (pc >= X::NP) prow[i] = 0x40000000;                              // no such piece: never in range, never committed
  }
  float st_stat = 0.f;                                 // thread t < QT: lse of query t; QT <= t < 2 QT: delta of query t - QT
  auto issue = [&](int q0) {
    const unsigned sq = (unsigned)q0 * (unsigned)a.q_stride * ES, sd = (unsigned)q0 * (unsigned)a.o_stride * ES;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const bool in = prow[i] < a.Nq - q0;                              // a query at or past Nq: zeros, by selection
      stq[i] = E::load_buf(rq, in ? qoff[i] + sq : OOB_OFF, 0);
      std_[i] = E::load_buf(rdo, in ? dooff[i] + sd : OOB_OFF, 0);
    }
    if (tid < 2 * QT) {
      const int qi = q0 + (tid % QT);
      st_stat = qi < a.Nq ? (tid < QT ? lsep[qi] : delp[qi]) : 0.f;     // (the P / dS of such a query are selected to zero below)
    }
  };
  auto commit = [&](int buf) {
    unsigned char* qb_ = lds + buf * BUF;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      if (tid + 256 * i < X::NP) {
        const int off = prow[i] * TP + psub[i] * 8 * ES;
        E::store(qb_ + off, stq[i]);
        E::store(qb_ + TB + off, std_[i]);
      }
    }
    if (tid < 2 * QT) ((float*)(qb_ + 2 * TB))[tid] = st_stat;
  };
  const int row_lane = r * TP + 8 * h * ES;
  const int t_lane = X::vt_lane_off(lane);

  issue(0);
  commit(0);
  if (QT < a.Nq) issue(QT);
  __syncthreads();
  for (int q0 = 0, cur = 0; q0 < a.Nq; q0 += QT, cur ^= 1) {
    const unsigned char* qb_ = lds + cur * BUF;
    const unsigned char* db = qb_ + TB;
    const float* lse_t = (const float*)(qb_ + 2 * TB);
    const float* del_t = lse_t + QT;
#pragma unroll
    for (int sub = 0; sub < QT / 32; ++sub) {
      if (q0 + sub * 32 < a.Nq) {                      // workgroup-uniform
        f32x16 s = (f32x16)(0.f), dp = (f32x16)(0.f);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          s = E::mma(E::load(qb_ + row_lane + sub * 32 * TP + ks * 16 * ES), kf[ks], s);     // S[query][key]
          dp = E::mma(E::load(db + row_lane + sub * 32 * TP + ks * 16 * ES), vf[ks], dp);    // dP[query][key]
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {                   // registers 4g..4g+3 <-> queries sub*32 + 8g + 4h + (0..3)
          const f32x4 l4 = *(const f32x4*)(lse_t + sub * 32 + 8 * g + 4 * h), d4 = *(const f32x4*)(del_t + sub * 32 + 8 * g + 4 * h);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = 4 * g + j;
            const float p = __builtin_amdgcn_exp2f(s[i] * kscale - l4[j]);
            s[i] = p;
            dp[i] = p * (dp[i] - d4[j]);                 // dS
          }
        }
        if (q0 + sub * 32 + 32 > a.Nq) {                // queries beyond Nq (workgroup-uniform): P = dS = 0, by selection
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (q0 + sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * h >= a.Nq) { s[i] = 0.f; dp[i] = 0.f; }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const Frag pf = D64<T>::pack_p(s, st), df = D64<T>::pack_p(dp, st);
          const unsigned char* dro = db + t_lane + (sub * 32 + 16 * st) * TP;
          const unsigned char* qro = qb_ + t_lane + (sub * 32 + 16 * st) * TP;
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) {
            dv[tt] = E::mma(X::load_vt(dro + tt * 32 * ES), pf, dv[tt]);
            dk[tt] = E::mma(X::load_vt(qro + tt * 32 * ES), df, dk[tt]);
          }
        }
      }
    }
    if (q0 + QT < a.Nq) {
      commit(cur ^ 1);
      if (q0 + 2 * QT < a.Nq) issue(q0 + 2 * QT);
    }
    __syncthreads();
  }
  if (key < a.Nkv) {
    const float sc = a.scale;
    T* dkd = (T*)a.dk + ((size_t)b * a.Nkv + key) * a.dkv_stride + head * D + 4 * h;
    T* dvd = (T*)a.dv + ((size_t)b * a.Nkv + key) * a.dkv_stride + head * D + 4 * h;
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
      for (int g = 0; g < 4; ++g)                        // register 4g + i <-> d = 32 tt + 8g + 4h + i; groups at d >= D are padding
        if (32 * tt + 8 * g < D) {
          store4(dkd + 32 * tt + 8 * g, dk[tt][4 * g] * sc, dk[tt][4 * g + 1] * sc, dk[tt][4 * g + 2] * sc, dk[tt][4 * g + 3] * sc);
          store4(dvd + 32 * tt + 8 * g, dv[tt][4 * g], dv[tt][4 * g + 1], dv[tt][4 * g + 2], dv[tt][4 * g + 3]);
        }
  }
}

template <typename T, int D>
static int launch_attn_hd_bwd(const pd_attn_hd_bwd_args* a, hipStream_t st) {
  using XB = HDB<T, D>;
  auto kq = attn_hd_dq_kernel<T, D>;
  auto kkv = attn_hd_dkv_kernel<T, D>;
  static LdsAttr attr_q, attr_kv;
  if (!ensure_lds(attr_q, kq, XB::LDS_DQ) || !ensure_lds(attr_kv, kkv, XB::LDS_DKV)) {
    set_error("pd_attn_hd_bwd: cannot reserve %d / %d bytes of LDS", XB::LDS_DQ, XB::LDS_DKV);
    return PD_ERR_LAUNCH;
  }
  const size_t nd = (size_t)a->B * a->Nq * a->heads;
  hipLaunchKernelGGL((attn_hd_delta_kernel<T, D>), dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, *a);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(kq, dim3(((a->Nq + 127) / 128) * a->heads * a->B), dim3(256), XB::LDS_DQ, st, *a);
  PD_LAUNCH_CHECK();
  hipLaunchKernelGGL(kkv, dim3(((a->Nkv + 127) / 128) * a->heads * a->B), dim3(256), XB::LDS_DKV, st, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

template <typename T>
static int dispatch_attn_hd_bwd(const pd_attn_hd_bwd_args* a, hipStream_t st) {
  if (a->D == 16) return launch_attn_hd_bwd<T, 16>(a, st);
  return launch_attn_hd_bwd<T, 32>(a, st);
}

}  // namespace pd

using namespace pd;

extern "C" int pd_attn_hd_bwd(const pd_attn_hd_bwd_args* a, void* stream) {
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_attn_hd_bwd: null args");
  PD_CHECK(a->D == 16 || a->D == 32, PD_ERR_SHAPE, "pd_attn_hd_bwd: head dimension %d not built (16, 32)", a->D);
  PD_CHECK(a->B > 0 && a->heads > 0 && a->Nq > 0 && a->Nkv > 0, PD_ERR_SHAPE, "pd_attn_hd_bwd: bad shape");
  PD_CHECK(a->q && a->k && a->v && a->o && a->dout && a->lse && a->delta && a->dq && a->dk && a->dv, PD_ERR_ARG, "pd_attn_hd_bwd: null pointer");
  PD_CHECK(a->scale == a->scale && a->scale != 0.f && a->scale - a->scale == 0.f, PD_ERR_ARG, "pd_attn_hd_bwd: scale must be finite and non-zero");
  const long long c = (long long)a->heads * a->D;
  PD_CHECK(c < (1ll << 28) && a->q_stride >= c && a->kv_stride >= c && a->o_stride >= c && a->dq_stride >= c && a->dkv_stride >= c &&
               a->q_stride % 8 == 0 && a->kv_stride % 8 == 0 && a->o_stride % 8 == 0 && a->dq_stride % 8 == 0 && a->dkv_stride % 8 == 0,
           PD_ERR_SHAPE, "pd_attn_hd_bwd: strides must cover heads*D channels and be multiples of 8");
  PD_CHECK((long long)((a->Nq + 127) / 128) * a->heads * a->B < (1ll << 31) && (long long)((a->Nkv + 127) / 128) * a->heads * a->B < (1ll << 31) &&
               ((long long)a->B * a->Nq * a->heads + 255) / 256 < (1ll << 31),
           PD_ERR_SHAPE, "pd_attn_hd_bwd: grid too large");
  // (the selected out-of-range offset OOB_OFF = 3 GiB must lie beyond every resource)
  PD_CHECK((unsigned long long)a->Nkv * (unsigned long long)a->kv_stride * 4ull < 0xC0000000ull &&
               (unsigned long long)a->Nq * (unsigned long long)(a->q_stride > a->o_stride ? a->q_stride : a->o_stride) * 4ull < 0xC0000000ull,
           PD_ERR_SHAPE, "pd_attn_hd_bwd: one sample's rows must span < 3 GiB (32-bit buffer offsets)");
  if (a->dtype == PD_F32) return dispatch_attn_hd_bwd<float>(a, (hipStream_t)stream);
  if (a->dtype == PD_BF16) return dispatch_attn_hd_bwd<bf16_t>(a, (hipStream_t)stream);
  if (a->dtype == PD_F16) return dispatch_attn_hd_bwd<half_t>(a, (hipStream_t)stream);
  set_error("pd_attn_hd_bwd: bad dtype");
  return PD_ERR_ARG;
}
