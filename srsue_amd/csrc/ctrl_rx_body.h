// ctrl_rx_body.h -- the arithmetic of the two-antenna DL control kernels (ctrl.hip pcfich_rx_kernel,
// pdcch_llr_rx_kernel, phich_rx_kernel), in a form that also compiles for the host (emu.cpp emu_pdcch_llr_rx), as
// demap_body.h does for the PDSCH demapper.  The control channels are equalised with the PDSCH demapper's
// maximum-ratio combining (demap_body.h eq_terms / eq_add / eq_finish: an antenna's terms formed as the one-antenna
// equalisers form them, added in antenna order, the regulariser or floor last):
//   1 port:  x = sum_a y_a h_a* / (sum_a |h_a|^2 + noise)
//   2 ports: hh = sum_a (|h00_a|^2 + |h11_a|^2) (<= 0 -> 1e-9),  x0 = sqrt2 sum_a (h00_a* r0_a + h11_a r1_a*) / hh,
//            x1 = sqrt2 sum_a (-h10_a r0_a* + h01_a* r1_a) / hh
// Antenna a's grid / estimates lie a * g_rx / a * c_rx float2 behind antenna 0's (mi_dl_batch_rx_stride).
#pragma once
#include "demap_body.h"

namespace mi {

// QPSK max-log soft bits, LLR > 0 => bit 1 (same scale as the PDSCH demapper)
__device__ __forceinline__ void qpsk_llr(float2 x, float* l) {
  const float a = 0.70710678118f;
  l[0] = ((x.x - a) * (x.x - a) - (x.x + a) * (x.x + a)) * 2.0f;
  l[1] = ((x.y - a) * (x.y - a) - (x.y + a) * (x.y + a)) * 2.0f;
}

// one RE of a one-port cell over NRX antennas; floor: the PHICH's 1e-9 floor on the summed denominator instead of
// the regulariser
template <int NRX, bool FLOOR>
__device__ __forceinline__ float2 eq_re_rx(const float2* __restrict__ g, const float2* __restrict__ c0, uint32_t r,
                                           float noise, size_t g_rx, size_t c_rx) {
  MI_FP_EXACT
  EqIn d;
  d.r0 = g[r];
  d.h00 = c0[r];
  EqAcc<false> acc = eq_terms<false>(d);
#pragma unroll
  for (int a = 1; a < NRX; a++) {
    d.r0 = g[a * g_rx + r];
    d.h00 = c0[a * c_rx + r];
    eq_add<false>(acc, d);
  }
  float2 x;
  if constexpr (FLOOR) {
    float den = acc.den;
    if (den <= 0.f) den = 1e-9f;
    x = make_float2(acc.nx / den, acc.ny / den);
  } else {
    eq_finish<false>(acc, noise, &x, nullptr);
  }
  return x;
}

// one SFBC RE pair (ra, rb) of a two-port cell over NRX antennas (c1: port 1's estimates of antenna 0)
template <int NRX>
__device__ __forceinline__ void eq_pair_rx(const float2* __restrict__ g, const float2* __restrict__ c0,
                                           const float2* __restrict__ c1, uint32_t ra, uint32_t rb, size_t g_rx,
                                           size_t c_rx, float2* x0, float2* x1) {
  EqAcc<true> acc = eq_terms<true>(EqIn{g[ra], g[rb], c0[ra], c0[rb], c1[ra], c1[rb]});
#pragma unroll
  for (int a = 1; a < NRX; a++) {
    const float2 *ga = g + a * g_rx, *p0 = c0 + a * c_rx, *p1 = c1 + a * c_rx;
    eq_add<true>(acc, EqIn{ga[ra], ga[rb], p0[ra], p0[rb], p1[ra], p1[rb]});
  }
  eq_finish<true>(acc, 0.0f, x0, x1);
}

// 4 REs of one REG / PCFICH quadruplet -> 4 equalised symbols
template <int NRX>
__device__ __forceinline__ void eq_quad_rx(const float2* __restrict__ g, const float2* __restrict__ c0,
                                           const float2* __restrict__ c1, const uint32_t* __restrict__ re, bool tm2,
                                           float noise, size_t g_rx, size_t c_rx, float2 (&x)[4]) {
  if (!tm2) {
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] = eq_re_rx<NRX, false>(g, c0, re[j], noise, g_rx, c_rx);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j += 2) eq_pair_rx<NRX>(g, c0, c1, re[j], re[j + 1], g_rx, c_rx, &x[j], &x[j + 1]);
  }
}

// the 8 soft bits of one PDCCH REG, descrambled with the 8 scrambling bits sw of its logical quadruplet, to o[0..7]
template <int NRX>
__device__ __forceinline__ void pdcch_reg_llr_rx(const float2* __restrict__ g, const float2* __restrict__ c0,
                                                 const float2* __restrict__ c1, const uint32_t* __restrict__ re,
                                                 bool tm2, float noise, size_t g_rx, size_t c_rx, uint32_t sw,
                                                 float* __restrict__ o) {
  float2 x[4];
  eq_quad_rx<NRX>(g, c0, c1, re, tm2, noise, g_rx, c_rx, x);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    float l[2];
    qpsk_llr(x[j], l);
    o[2 * j] = ((sw >> (2 * j)) & 1u) ? -l[0] : l[0];
    o[2 * j + 1] = ((sw >> (2 * j + 1)) & 1u) ? -l[1] : l[1];
  }
}

}  // namespace mi
