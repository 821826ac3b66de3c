// pucch.hip -- PUCCH formats 1/1a/1b and 2/2a/2b on gfx950 (36.211 5.4, 5.5.2.2, 5.6; normal CP).
//
//   pucch_kernel   one workgroup per (transmission, SC-FDMA symbol).  A PUCCH symbol has 12 non-zero
//                  subcarriers, each exp(j pi i / 12) for an integer i: the base sequence contributes 3 phi(k),
//                  the cyclic shift 2 n_cs k, and the symbol's factor -- d(0) S(ns) w(m) for formats 1x, the QPSK
//                  symbol d(n) or the DMRS factor for formats 2x -- one offset common to the 12.  The
//                  time-domain sample is therefore evaluated directly,
//                    s(n) = exp(j pi (2 k0 + 1) n / N) / sqrt(N) . sum_k c_k w^k,  w = exp(j 2 pi n / N),
//                  by Horner's rule on the 12 coefficients held in registers: no transform, no LDS, no barrier.
//                  The tail (half-subcarrier shift, cyclic prefix, scale, cfo) is that of pusch_mod_kernel.
#include <hip/hip_runtime.h>

#include "pucch.h"
#include "ul_seq_dev.h"

namespace mi {

namespace {

// phase index (units of pi / 12) of the 1a / 1b constellation: 1 bit 0 -> 1, 1 -> -1; 2 bits (b0 b1) 00 -> 1,
// 01 -> -j, 10 -> j, 11 -> -1 (36.211 Table 5.4.1-1)
__device__ __forceinline__ uint32_t ack_phase(uint32_t two_bits, uint32_t b0, uint32_t b1) {
  if (!two_bits) return b0 ? 12u : 0u;
  return b0 ? (b1 ? 12u : 6u) : (b1 ? 18u : 0u);
}

}  // namespace

__global__ __launch_bounds__(PUCCH_THREADS) void pucch_kernel(const MiPucchTx* __restrict__ txs,
                                                              const uint32_t* __restrict__ rm,
                                                              const uint32_t* __restrict__ uci,
                                                              float2* __restrict__ iq) {
  const MiPucchTx x = txs[blockIdx.x];
  const uint32_t word = uci[blockIdx.x];
  const uint32_t l = blockIdx.y, slot = l / 7, ls = l % 7, t = threadIdx.x, N = x.N;
  const uint32_t b0 = word & 1u, b1 = (word >> 1) & 1u;
  const uint32_t n_oc = slot ? x.n_oc[1] : x.n_oc[0];   // selects, no dynamic struct index
  // the symbol's common factor as a phase index a (units of pi / 12), or nothing sent
  uint32_t a = 0;
  bool zero = false;
  if (x.format <= MI_PUCCH_1B) {
    if (ls >= 2 && ls <= 4) {   // DMRS (5.5.2.2.1): w-bar_noc(m) = omega^(n_oc m), omega = exp(j 2 pi / 3)
      a = 8u * ((n_oc * (ls - 2)) % 3u);
    } else {
      const uint32_t m = ls < 2 ? ls : ls - 3;   // data symbols 0, 1, 5, 6 -> m = 0..3
      const bool shrt = x.shortened && slot == 1;
      if (shrt && m == 3) {
        zero = true;
      } else if (shrt) {        // N_SF = 3: the DFT covers
        a = 8u * ((n_oc * m) % 3u);
      } else {                  // N_SF = 4: [+ + + +], [+ - + -], [+ - - +]
        const bool neg = n_oc == 1 ? (m & 1u) != 0 : n_oc == 2 ? (m == 1 || m == 2) : false;
        a = neg ? 12u : 0u;
      }
      if (x.format != MI_PUCCH_1) a += ack_phase(x.format == MI_PUCCH_1B, b0, b1);   // d(0)
      if (slot ? x.s_odd[1] : x.s_odd[0]) a += 6u;                                       // S(ns) = j
    }
  } else {
    if (ls == 1 || ls == 5) {   // DMRS (5.5.2.2.1): the second one of each slot carries d(10) in 2a / 2b
      if (ls == 5 && x.format != MI_PUCCH_2) a = ack_phase(x.format == MI_PUCCH_2B, b0, b1);
    } else {
      // (20, A) block code (36.212 5.2.3.3), scrambling (36.211 5.4.2), QPSK (7.1.2): bit i at bit 31 - i
      uint32_t cw = x.scr;
      for (uint32_t k = 0; k < x.cqi_len && k < (uint32_t)PUCCH_NCOL; k++)
        if ((word >> (8 + k)) & 1u) cw ^= rm[k];
      const uint32_t d = 5 * slot + (ls == 0 ? 0u : ls == 6 ? 4u : ls - 1);   // d(0..9)
      const uint32_t q0 = (cw >> (31 - 2 * d)) & 1u, q1 = (cw >> (30 - 2 * d)) & 1u;
      a = q0 ? (q1 ? 15u : 9u) : (q1 ? 21u : 3u);
    }
  }
  const uint32_t cp = (uint32_t)cp_len((int)N, (int)ls);
  const uint32_t pos = (uint32_t)(symbol_offset((int)N, (int)l)) - cp;   // first sample of symbol l (its CP)
  float2* dst = iq + x.iq_off + pos;
  if (zero) {
    for (uint32_t i = t; i < N + cp; i += PUCCH_THREADS) dst[i] = make_float2(0.0f, 0.0f);
    return;
  }
  // c_k = exp(j pi (3 phi_u(k) + 2 n_cs k + a) / 12)
  const uint32_t u = slot ? x.u[1] : x.u[0];
  const uint32_t ncs = ((slot ? x.ncs[1] : x.ncs[0]) >> (4 * ls)) & 15u;
  float2 c[12];
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const uint32_t idx = (uint32_t)(3 * (int)UL_PHI12[u][k] + 24) + 2u * ncs * (uint32_t)k + a;
    float sv, cv;
    sincospif((float)(idx % 24u) * (1.0f / 12.0f), &sv, &cv);
    c[k] = make_float2(cv, sv);
  }
  // subcarrier k of the PRB sits at frequency (12 n_prb + k - W / 2 + 1 / 2) df (5.6)
  const int k0 = (int)(12 * (slot ? x.n_prb[1] : x.n_prb[0])) - (int)(x.W / 2);
  const int twoN = 2 * (int)N;
  const float gN = rsqrtf((float)N) * x.scale, rN = 1.0f / (float)N;
  for (uint32_t i = t; i < N + cp; i += PUCCH_THREADS) {
    const int n = (int)i - (int)cp;
    const uint32_t nm = (uint32_t)(n + (int)N) % N;
    float sv, cv;
    sincospif(2.0f * (float)nm * rN, &sv, &cv);
    const float2 w = make_float2(cv, sv);
    float2 acc = c[11];
#pragma unroll
    for (int k = 10; k >= 0; k--) {
      acc = cmul(acc, w);
      acc.x += c[k].x;
      acc.y += c[k].y;
    }
    dst[i] = sc_shift_out(acc, 2 * k0 + 1, n, twoN, x.cfo, pos + i, rN, gN);
  }
}

void launch_pucch(const MiPucchTx* txs, uint32_t n_tx, const uint32_t* rm, const uint32_t* uci, float2* iq,
                  hipStream_t st) {
  if (!n_tx) return;
  hipLaunchKernelGGL(pucch_kernel, dim3(n_tx, 14), dim3(PUCCH_THREADS), 0, st, txs, rm, uci, iq);
}

}  // namespace mi
