// pd_attn_hd: softmax(q k^T * scale) v for the head dimensions between the dedicated kernels: D = 16 / 32 (attention_head_dim 16 / 32 of the
// pixel UNet) and D = 40 / 80 / 160 (the Stable-Diffusion 1.x denoisers: 8 heads on 320 / 640 / 1280 channels).  The structure is attn_d64_kernel's one-fragment form (sd_kernels.hip):
// workgroup = 4 waves = 128 queries of one (batch, head), keys / values stream through LDS in double-buffered tiles, per wave and
// 32-key sub-tile
//   S^T[key][query] = K[32 x DK] . Q^T[DK x 32]       DK / 16 MFMA k-steps, DK = D rounded up to 16 (40 -> 48: 3 steps, not the 4 of a 64-padded head)
//   deferred-rescale online softmax, P in registers
//   O^T[d][query] += V^T[DV x 32 keys] . P^T          DV / 32 row tiles, DV = D rounded up to 32 (80 -> 96: 3 tiles, not the 4 of a 128-padded head)
// D = 32 has no padding at all; D = 16 has one k-step and one row tile whose upper half is padding (never stored).
// The padding of D exists in LDS and registers only, as zeros: the pad columns of the K / V tiles are zeroed once per workgroup (the staging
// never writes them), the pad elements of the Q fragments are selected to zero.  Nothing is read from HBM for them (the channels behind a head
// belong to the next head, or to nobody).
// Keys >= Nkv: their staging pieces are SELECTED to an offset beyond any resource (zeros), whatever the range check of the buffer instruction
// covers ("Buffer-resource bounds"), and their scores are selected to -inf; queries >= Nq re-read the last query and are not stored.
#include <stdlib.h>
#include "pd_common.h"
#include "pd_stage.h"
#include "pd_hd.h"

namespace pd {

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_hd_kernel(const pd_attn_hd_args a) {
  using E = Elem<T>;
  using Frag = typename E::Frag;
  using X = HD<T, D>;
  constexpr int KT = X::KT, KP = X::KP, VP = X::VP, ES = X::ES, KS = X::KS, NT = X::NT, PPR = X::PPR, PIECES = X::PIECES;
  constexpr int KBYTES = X::KBYTES, VBYTES = X::VBYTES;
  constexpr int QPB = 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // [2][K tile | V tile]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nqb = (a.Nq + QPB - 1) / QPB;
  const int total = nqb * a.heads * a.B;
  const int item = xcd_chunk_index(blockIdx.x, total);                  // query blocks of one head share an XCD / L2
  const int qb = item % nqb, head = (item / nqb) % a.heads, b = item / (nqb * a.heads);
  const T* qp = (const T*)a.q + (size_t)b * a.Nq * a.q_stride + head * D;
  const T* kp = (const T*)a.k + (size_t)b * a.Nkv * a.kv_stride + head * D;
  const T* vp = (const T*)a.v + (size_t)b * a.Nkv * a.kv_stride + head * D;

  // zeros in the pad columns of both buffers (K: D .. DK, V: D .. DV); the staging below writes columns < D only
  if (tid < 2 * KT) {
    unsigned char* kb = lds + (tid / KT) * (KBYTES + VBYTES) + (tid % KT) * KP;
    unsigned char* vb = lds + (tid / KT) * (KBYTES + VBYTES) + KBYTES + (tid % KT) * VP;
#pragma unroll
    for (int o = D * ES; o < X::DK * ES; o += 16) *(u32x4*)(kb + o) = (u32x4)(0u);
#pragma unroll
    for (int o = D * ES; o < X::DV * ES; o += 16) *(u32x4*)(vb + o) = (u32x4)(0u);
  }

  // Q^T fragments (B operand): lane (query, h), k-step ks: d = 16 ks + 8 h + j, as stored; d >= D: zeros.  The scale (x log2 e) is applied to
  // the fp32 scores, not to q: a 16-bit q * scale is rounded a second time, and with few keys that rounding IS the error of the lse
  // (one key, D = 40, bf16: 2.2e-3 relative, against the 2e-3 bound of pd_attn_d64's lse; the products of stored 16-bit values are exact in fp32).
  const float qscale = a.scale * 1.4426950408889634f;
  const int query = qb * QPB + wave * 32 + r;
  Frag qf[KS];
  {
    const int qc = min(query, a.Nq - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = 16 * ks + 8 * h;
      const bool real = d0 < D;                                          // (D is a multiple of 8: a piece is real or padding as a whole)
      qf[ks] = E::load(qp + (size_t)qc * a.q_stride + (real ? d0 : 0));
      if (!real) qf[ks] = E::zero();
    }
  }
  // Deferred-rescale online softmax, as attn_d64_kernel: `m` is a REFERENCE maximum (log2 domain) shared by both lane halves of a query,
  // p = exp2(s - m); it is raised only when a score of the sub-tile exceeds m + RESCALE_THR (the first sub-tile takes the exact maximum),
  // so p <= 2^THR -- 256, inside fp16 as well.  s = raw * qscale - m is one fma per score.
  constexpr float RESCALE_THR = 8.0f;
  f32x16 o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o[t] = (f32x16)(0.f);
  float m = 0.f, l = 0.f;                                                // l: this lane half's share of the row sum
  bool first = true;

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
    unsigned char* kb = lds + buf * (KBYTES + VBYTES);
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      if (tid + 256 * i < X::NP) {
        const int row = prow[i], sub = psub[i];
        E::store(kb + row * KP + sub * 8 * ES, stk[i]);
        E::store(kb + KBYTES + row * VP + sub * 8 * ES, stv[i]);
      }
    }
  };
  const int k_lane = r * KP + 8 * h * ES;             // K row fragment: key r, d = 16 ks + 8 h + (0..7)
  const int v_lane = X::vt_lane_off(lane);

  issue(0);
  commit(0);
  if (KT < a.Nkv) issue(KT);
  __syncthreads();
  for (int k0 = 0, cur = 0; k0 < a.Nkv; k0 += KT, cur ^= 1) {
    const unsigned char* kb = lds + cur * (KBYTES + VBYTES);
    const unsigned char* vb = kb + KBYTES;
#pragma unroll
    for (int sub = 0; sub < KT / 32; ++sub) {
      if (k0 + sub * 32 < a.Nkv) {                    // workgroup-uniform
        f32x16 s;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const Frag kf = E::load(kb + k_lane + sub * 32 * KP + ks * 16 * ES);
          s = E::mma(kf, qf[ks], ks == 0 ? (f32x16)(0.f) : s);
        }
        s = s * qscale - m;                             // log2-domain scores against the reference maximum
        if (k0 + sub * 32 + 32 > a.Nkv) {              // keys beyond the context length
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (k0 + sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * h >= a.Nkv) s[i] = -INFINITY;
        }
        float t = fmaxf(fmaxf(s[0], s[1]), s[2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2) t = fmaxf(fmaxf(t, s[i]), s[i + 1]);
        t = fmaxf(t, s[15]);
        if (__builtin_amdgcn_ballot_w64(first || t > RESCALE_THR) != 0) {
          const float tq = fmaxf(t, __shfl_xor(t, 32));          // finite: every sub-tile visited holds at least one real key
          const float delta = first ? tq : fmaxf(0.f, tq);       // how far the reference moves up (first: to the exact maximum)
          const float alpha = first ? 0.f : __builtin_amdgcn_exp2f(-delta);    // first: l = o = 0 (and exp2 of a very negative maximum's negation is inf)
          m += delta;
          l *= alpha;
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) o[tt] *= alpha;
          s -= delta;
          first = false;
        }
        f32x2 acc2 = (f32x2)(0.f);
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          f32x2 d;
          d.x = __builtin_amdgcn_exp2f(s[i]); d.y = __builtin_amdgcn_exp2f(s[i + 1]);
          s[i] = d.x; s[i + 1] = d.y;
          acc2 += d;
        }
        l += acc2.x + acc2.y;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const Frag pf = D64<T>::pack_p(s, st);
          const unsigned char* vs = vb + v_lane + (sub * 32 + 16 * st) * VP;
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) o[tt] = E::mma(X::load_vt(vs + tt * 32 * ES), pf, o[tt]);
        }
      }
    }
    if (k0 + KT < a.Nkv) {
      commit(cur ^ 1);
      if (k0 + 2 * KT < a.Nkv) issue(k0 + 2 * KT);
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32);
  if (query < a.Nq) {
    const float inv = 1.0f / l;
    if (a.lse && h == 0) a.lse[((size_t)b * a.heads + head) * a.Nq + query] = m + __log2f(l);     // log2 domain, scale included
    T* dst = (T*)a.out + ((size_t)b * a.Nq + query) * a.out_stride + head * D + 4 * h;
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
      for (int g = 0; g < 4; ++g)                        // register 4g + i <-> d = 32 tt + 8g + 4h + i; groups at d >= D are padding
        if (32 * tt + 8 * g < D)
          store4(dst + 32 * tt + 8 * g, o[tt][4 * g] * inv, o[tt][4 * g + 1] * inv, o[tt][4 * g + 2] * inv, o[tt][4 * g + 3] * inv);
  }
}

template <typename T, int D>
static int launch_attn_hd(const pd_attn_hd_args* a, hipStream_t st) {
  constexpr int LDS = HD<T, D>::LDS;
  auto kern = attn_hd_kernel<T, D>;
  static LdsAttr attr;
  if (!ensure_lds(attr, kern, LDS)) {
    set_error("pd_attn_hd: cannot reserve %d bytes of LDS", LDS);
    return PD_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(((a->Nq + 127) / 128) * a->heads * a->B), dim3(256), LDS, st, *a);
  PD_LAUNCH_CHECK();
  return PD_OK;
}

template <typename T>
static int dispatch_attn_hd(const pd_attn_hd_args* a, hipStream_t st) {
  if (a->D == 16) return launch_attn_hd<T, 16>(a, st);
  if (a->D == 32) return launch_attn_hd<T, 32>(a, st);
  if (a->D == 40) return launch_attn_hd<T, 40>(a, st);
  if (a->D == 80) return launch_attn_hd<T, 80>(a, st);
  return launch_attn_hd<T, 160>(a, st);
}

}  // namespace pd

using namespace pd;

extern "C" int pd_attn_hd(const pd_attn_hd_args* a, void* stream) {
  PD_CHECK(a != nullptr, PD_ERR_ARG, "pd_attn_hd: null args");
  PD_CHECK(a->D == 16 || a->D == 32 || a->D == 40 || a->D == 80 || a->D == 160, PD_ERR_SHAPE,
           "pd_attn_hd: head dimension %d not built (16, 32, 40, 80, 160)", a->D);
  PD_CHECK(a->B > 0 && a->heads > 0 && a->Nq > 0 && a->Nkv > 0, PD_ERR_SHAPE, "pd_attn_hd: bad shape");
  PD_CHECK(a->q && a->k && a->v && a->out, PD_ERR_ARG, "pd_attn_hd: null pointer");
  PD_CHECK(a->scale == a->scale && a->scale != 0.f && a->scale - a->scale == 0.f, PD_ERR_ARG, "pd_attn_hd: scale must be finite and non-zero");
  PD_CHECK((long long)a->heads * a->D < (1ll << 28) && a->q_stride >= a->heads * a->D && a->kv_stride >= a->heads * a->D &&
               a->out_stride >= a->heads * a->D && a->q_stride % 8 == 0 && a->kv_stride % 8 == 0 && a->out_stride % 8 == 0,
           PD_ERR_SHAPE, "pd_attn_hd: strides must cover heads*D channels and be multiples of 8");
  PD_CHECK((long long)((a->Nq + 127) / 128) * a->heads * a->B < (1ll << 31), PD_ERR_SHAPE, "pd_attn_hd: grid too large");
  // (the selected out-of-range offset OOB_OFF = 3 GiB must lie beyond every resource)
  PD_CHECK((unsigned long long)a->Nkv * (unsigned long long)a->kv_stride * 4ull < 0xC0000000ull, PD_ERR_SHAPE,
           "pd_attn_hd: one sample's K / V rows must span < 3 GiB (32-bit buffer offsets)");
  if (a->dtype == PD_F32) return dispatch_attn_hd<float>(a, (hipStream_t)stream);
  if (a->dtype == PD_BF16) return dispatch_attn_hd<bf16_t>(a, (hipStream_t)stream);
  if (a->dtype == PD_F16) return dispatch_attn_hd<half_t>(a, (hipStream_t)stream);
  set_error("pd_attn_hd: bad dtype");
  return PD_ERR_ARG;
}
