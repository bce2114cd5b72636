// Microbenchmark (round 3): issue cost of the candidates for the d = 8 attention's exponentials and conversions on gfx950 --
// v_exp_f32 vs v_exp_f16 (is the 16-bit transcendental any cheaper?), v_cvt_pk_bf16_f32, v_cvt_pk_f16_f32 (v_cvt_pkrtz),
// v_pk_mul_f16, v_pk_fma_f32.  One wave per SIMD would hide nothing, so 4 waves per SIMD issue independent streams; the
// figure printed is SIMD-cycles (at 2.4 GHz nominal) per wave-instruction.
// Round 26: the truncating-pack candidates beside v_perm_b32 (v_pack_b32_f16 with op_sel, v_mov_b32 SDWA in place), each also
// interleaved 1 : 2 with v_exp_f32 as in the attention tile, and a bit check of all 65 536 half patterns through each of them.
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/exp_variants scripts/micro/exp_variants.hip && /tmp/exp_variants
#include <hip/hip_runtime.h>
#include <stdio.h>

#define REP16(X) X X X X X X X X X X X X X X X X

template <int MODE>
__global__ __launch_bounds__(256) void k(float* out, int iters) {
  float a0 = threadIdx.x * 1e-3f, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
  for (int it = 0; it < iters; ++it) {
    if (MODE == 0) {
      REP16(asm volatile("v_exp_f32 %0, %0\n v_exp_f32 %1, %1\n v_exp_f32 %2, %2\n v_exp_f32 %3, %3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));)
    } else if (MODE == 1) {
      REP16(asm volatile("v_exp_f16 %0, %0\n v_exp_f16 %1, %1\n v_exp_f16 %2, %2\n v_exp_f16 %3, %3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));)
    } else if (MODE == 2) {
      REP16(asm volatile("v_cvt_pk_bf16_f32 %0, %4, %5\n v_cvt_pk_bf16_f32 %1, %5, %6\n v_cvt_pk_bf16_f32 %2, %6, %7\n v_cvt_pk_bf16_f32 %3, %7, %4"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 3) {
      REP16(asm volatile("v_cvt_pkrtz_f16_f32 %0, %4, %5\n v_cvt_pkrtz_f16_f32 %1, %5, %6\n v_cvt_pkrtz_f16_f32 %2, %6, %7\n v_cvt_pkrtz_f16_f32 %3, %7, %4"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 4) {
      REP16(asm volatile("v_pk_mul_f16 %0, %0, %4\n v_pk_mul_f16 %1, %1, %5\n v_pk_mul_f16 %2, %2, %6\n v_pk_mul_f16 %3, %3, %7"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 5) {
      REP16(asm volatile("v_fma_f32 %0, %0, %4, %5\n v_fma_f32 %1, %1, %5, %6\n v_fma_f32 %2, %2, %6, %7\n v_fma_f32 %3, %3, %7, %4"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 6) {       // exp + cvt interleaved: do they share an issue port?
      REP16(asm volatile("v_exp_f32 %0, %0\n v_cvt_pk_bf16_f32 %2, %4, %5\n v_exp_f32 %1, %1\n v_cvt_pk_bf16_f32 %3, %6, %7"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 7) {       // exp + fma interleaved
      REP16(asm volatile("v_exp_f32 %0, %0\n v_fma_f32 %2, %2, %4, %5\n v_exp_f32 %1, %1\n v_fma_f32 %3, %3, %6, %7"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 8) {       // v_ldexp_f32 (scale by 2^n: the cheap half of a split exponential)
      REP16(asm volatile("v_ldexp_f32 %0, %0, %4\n v_ldexp_f32 %1, %1, %5\n v_ldexp_f32 %2, %2, %6\n v_ldexp_f32 %3, %3, %7"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 10) {      // v_perm_b32: the upper halves of two fp32 words = a truncating bf16 pack
      REP16(asm volatile("v_perm_b32 %0, %4, %5, %8\n v_perm_b32 %1, %5, %6, %8\n v_perm_b32 %2, %6, %7, %8\n v_perm_b32 %3, %7, %4, %8"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7), "s"(0x07060302u));)
    } else if (MODE == 11) {      // v_pack_b32_f16 with op_sel on both sources: the same two upper halves, as f16 operands
      REP16(asm volatile("v_pack_b32_f16 %0, %4, %5 op_sel:[1,1,0]\n v_pack_b32_f16 %1, %5, %6 op_sel:[1,1,0]\n v_pack_b32_f16 %2, %6, %7 op_sel:[1,1,0]\n v_pack_b32_f16 %3, %7, %4 op_sel:[1,1,0]"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 12) {      // v_mov_b32 SDWA: upper half of the source into the lower half of the register that holds `hi`, in place
      REP16(asm volatile("v_mov_b32_sdwa %0, %4 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n v_mov_b32_sdwa %1, %5 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n"
                         " v_mov_b32_sdwa %2, %6 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n v_mov_b32_sdwa %3, %7 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 13) {      // the tile body's mix: two exponentials per pack (v_perm_b32)
      REP16(asm volatile("v_exp_f32 %0, %0\n v_exp_f32 %1, %1\n v_perm_b32 %2, %6, %7, %8\n v_exp_f32 %4, %4\n v_exp_f32 %5, %5\n v_perm_b32 %3, %7, %6, %8"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5) : "v"(a6), "v"(a7), "s"(0x07060302u));)
    } else if (MODE == 14) {      // ... v_pack_b32_f16
      REP16(asm volatile("v_exp_f32 %0, %0\n v_exp_f32 %1, %1\n v_pack_b32_f16 %2, %6, %7 op_sel:[1,1,0]\n v_exp_f32 %4, %4\n v_exp_f32 %5, %5\n v_pack_b32_f16 %3, %7, %6 op_sel:[1,1,0]"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5) : "v"(a6), "v"(a7));)
    } else if (MODE == 15) {      // ... v_mov_b32 SDWA
      REP16(asm volatile("v_exp_f32 %0, %0\n v_exp_f32 %1, %1\n v_mov_b32_sdwa %2, %6 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n"
                         " v_exp_f32 %4, %4\n v_exp_f32 %5, %5\n v_mov_b32_sdwa %3, %7 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5) : "v"(a6), "v"(a7));)
    } else if (MODE == 16) {      // two exponentials only, same registers as the three mixes (their base line)
      REP16(asm volatile("v_exp_f32 %0, %0\n v_exp_f32 %1, %1\n v_exp_f32 %2, %2\n v_exp_f32 %3, %3" : "+v"(a0), "+v"(a1), "+v"(a4), "+v"(a5));)
    } else if (MODE == 17) {      // a wait state behind every pack (the 2 wait states a VALU result needs before an MFMA reads it)
      REP16(asm volatile("v_perm_b32 %0, %4, %5, %8\n s_nop 0\n v_perm_b32 %1, %5, %6, %8\n s_nop 0\n v_perm_b32 %2, %6, %7, %8\n s_nop 0\n v_perm_b32 %3, %7, %4, %8\n s_nop 0"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7), "s"(0x07060302u));)
    } else if (MODE == 18) {      // a lane-varying address add (what every 32-key sub-tile pays for its K fragment address)
      REP16(asm volatile("v_add_u32 %0, %0, %4\n v_add_u32 %1, %1, %5\n v_add_u32 %2, %2, %6\n v_add_u32 %3, %3, %7"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7));)
    } else if (MODE == 9) {       // v_pk_fma_f32
      double d0 = a0, d1 = a1, d2 = a2, d3 = a3, d4 = a4, d5 = a5;
      REP16(asm volatile("v_pk_fma_f32 %0, %0, %4, %5\n v_pk_fma_f32 %1, %1, %5, %4\n v_pk_fma_f32 %2, %2, %4, %5\n v_pk_fma_f32 %3, %3, %5, %4"
                         : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(d4), "v"(d5));)
      a0 += (float)d0; a1 += (float)d1; a2 += (float)d2; a3 += (float)d3;
    }
  }
  out[blockIdx.x * 256 + threadIdx.x] = a0 + a1 + a2 + a3;
}
template <int MODE> void run(const char* name, int per_iter = 64) {
  float* d; (void)hipMalloc(&d, 256 * 4096 * 4);
  int iters = 1000;
  k<MODE><<<256 * 4, 256>>>(d, 10);
  (void)hipDeviceSynchronize();
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0); k<MODE><<<256 * 4, 256>>>(d, iters); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
  float ms; (void)hipEventElapsedTime(&ms, e0, e1);
  // 1024 workgroups of 4 waves on 256 CUs = 4 workgroups per CU = 4 waves per SIMD; each wave issues iters * per_iter vector instructions
  double per_simd_instr = 4.0 * iters * per_iter;
  double cyc = ms * 1e-3 * 2.4e9;
  printf("%-44s %.3f ms: %.2f SIMD-cycles@2.4GHz per wave-instruction\n", name, ms, cyc / per_simd_instr);
  (void)hipFree(d);
}
// Bit check of the truncating-pack candidates: every 16-bit pattern as the upper half of `lo` and of `hi` (the lower halves hold junk) must
// come out as (bits(hi) & 0xffff0000) | (bits(lo) >> 16).  Classes by the f16 VIEW of the half: denormal (exponent field 0, mantissa != 0: a
// bf16 below 2^-119), NaN (exponent field 31, mantissa != 0: a bf16 exponent of 0xF8 or more), everything else.
template <int WHICH>
__global__ void pack_bits(uint32_t* out) {
  const uint32_t pat = blockIdx.x * 256 + threadIdx.x;              // 0 .. 65535
  const uint32_t lo = (pat << 16) | 0x5a5au, hi = ((pat * 40503u) << 16) | 0xa5a5u;
  uint32_t d;
  if (WHICH == 0) asm volatile("v_perm_b32 %0, %2, %1, %3" : "=v"(d) : "v"(lo), "v"(hi), "s"(0x07060302u));
  else if (WHICH == 1) asm volatile("v_pack_b32_f16 %0, %1, %2 op_sel:[1,1,0]" : "=v"(d) : "v"(lo), "v"(hi));
  else { d = hi; asm volatile("v_mov_b32_sdwa %0, %1 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1" : "+v"(d) : "v"(lo)); }
  out[pat] = d;
}
template <int WHICH> void bits(const char* name) {
  uint32_t* d; (void)hipMalloc(&d, 65536 * 4);
  static uint32_t h[65536];
  pack_bits<WHICH><<<256, 256>>>(d);
  (void)hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
  int bad[3] = {0, 0, 0}, n[3] = {0, 0, 0};
  for (uint32_t pat = 0; pat < 65536; ++pat) {
    const uint32_t lo16 = pat, hi16 = (pat * 40503u) & 0xffffu;
    const uint32_t want = (hi16 << 16) | lo16;
    auto cls = [](uint32_t x) { const uint32_t e = (x >> 10) & 31, m = x & 1023; return e == 0 && m ? 0 : e == 31 && m ? 1 : 2; };
    const int cl = cls(lo16), ch = cls(hi16);
    n[cl]++; n[ch]++;
    if ((h[pat] & 0xffffu) != (want & 0xffffu)) bad[cl]++;
    if ((h[pat] >> 16) != (want >> 16)) bad[ch]++;
  }
  printf("bits %-20s altered halves: f16-view denormal %d / %d, f16-view NaN %d / %d, other %d / %d\n", name, bad[0], n[0], bad[1], n[1], bad[2], n[2]);
  (void)hipFree(d);
}
int main() {
  run<0>("v_exp_f32");
  run<1>("v_exp_f16");
  run<2>("v_cvt_pk_bf16_f32");
  run<3>("v_cvt_pkrtz_f16_f32");
  run<4>("v_pk_mul_f16");
  run<5>("v_fma_f32");
  run<6>("v_exp_f32 + v_cvt_pk_bf16_f32 (1:1)");
  run<7>("v_exp_f32 + v_fma_f32 (1:1)");
  run<8>("v_ldexp_f32");
  run<9>("v_pk_fma_f32");
  run<10>("v_perm_b32");
  run<11>("v_pack_b32_f16 op_sel:[1,1,0]");
  run<12>("v_mov_b32_sdwa WORD_1 -> WORD_0, in place");
  run<16>("v_exp_f32 (registers of the 2:1 mixes)");
  run<13>("v_exp_f32 x2 + v_perm_b32 (2:1)", 96);
  run<14>("v_exp_f32 x2 + v_pack_b32_f16 (2:1)", 96);
  run<15>("v_exp_f32 x2 + v_mov_b32_sdwa (2:1)", 96);
  run<17>("v_perm_b32 + s_nop 0 (per pair)");
  run<18>("v_add_u32");
  bits<0>("v_perm_b32");
  bits<1>("v_pack_b32_f16");
  bits<2>("v_mov_b32_sdwa");
  return 0;
}
