// demap_body.h -- equalisation + max-log soft demapping arithmetic shared by demap_kernel (demap.hip)
// and the fused demap -> rate de-matching path of rm_combine_kernel (rm.hip), so both produce the
// same LLRs (srslte_predecoding_single / _diversity + srslte_demod_soft_demodulate with sigma^2 = 0.5 +
// srslte_scrambling_f, inside srslte_pdsch_decode_rnti, /root/reference/ue/src/phy/phch_worker.cc:347).
#pragma once
#include "dl_common.h"
#if defined(MI_EMU)
#define __forceinline__ inline   // host emulation build (emu.cpp emu_pdsch_llr_rx): the same arithmetic with g++
#endif

namespace mi {

// Equalisation, shared by every path that forms LLRs (demap_kernel, the fused staging and the direct form of
// rate de-matching, the single-LLR repetition path), so that all give the same floats.  Floating-point
// contraction is off here: the default (fast) lets the compiler fuse a multiply into an add or not depending
// on the surrounding code, which made two of these paths differ in the last bits; uncontracted, the
// arithmetic is also the oracle's (plain C, no FMA).
#if defined(__clang__)
#define MI_FP_EXACT _Pragma("clang fp contract(off)")
#else
#define MI_FP_EXACT
#endif
// TM1 MMSE, one antenna: y h* / (|h|^2 + noise)
__device__ __forceinline__ float2 eq_single(float2 y, float2 h, float noise) {
  MI_FP_EXACT
  const float den = h.x * h.x + h.y * h.y + noise;
  return make_float2((y.x * h.x + y.y * h.y) / den, (y.y * h.x - y.x * h.y) / den);
}
// TM2 SFBC (Alamouti) pair, one antenna: symbols x0 (k = 0) and x1 (k = 1) of REs ra / rb
__device__ __forceinline__ void eq_sfbc(float2 r0, float2 r1, float2 h00, float2 h01, float2 h10, float2 h11,
                                       float2* x0, float2* x1) {
  MI_FP_EXACT
  float hh = h00.x * h00.x + h00.y * h00.y + h11.x * h11.x + h11.y * h11.y;
  if (hh <= 0.f) hh = 1e-9f;
  const float sc = 1.41421356237309504880f / hh;
  *x0 = make_float2(sc * ((h00.x * r0.x + h00.y * r0.y) + (h11.x * r1.x + h11.y * r1.y)),
                    sc * ((h00.x * r0.y - h00.y * r0.x) + (h11.y * r1.x - h11.x * r1.y)));
  *x1 = make_float2(sc * (-(h10.x * r0.x + h10.y * r0.y) + (h01.x * r1.x + h01.y * r1.y)),
                    sc * (-(h10.y * r0.x - h10.x * r0.y) + (h01.x * r1.y - h01.y * r1.x)));
}
// Receive diversity: maximum-ratio combining over the receive antennas, for every path that forms LLRs.
//   TM1 MMSE: x = sum_a y_a h_a* / (sum_a |h_a|^2 + noise)
//   TM2 SFBC pair: hh = sum_a (|h00_a|^2 + |h11_a|^2),  x0 = sqrt2 sum_a (h00_a* r0_a + h11_a r1_a*) / hh,
//                  x1 = sqrt2 sum_a (-h10_a r0_a* + h01_a* r1_a) / hh     (hh <= 0 -> 1e-9 after the sum)
// An antenna's terms (eq_terms) are formed exactly as eq_single / eq_sfbc form them, added in antenna order
// (eq_add), the regulariser last (eq_finish): with one antenna the result is eq_single's / eq_sfbc's floats, and the
// one-antenna instantiations call those two directly (the same instructions as before receive diversity).  The
// caller loads one antenna's inputs at a time, so no two antennas' six values are live at once:
//   EqAcc<TM2> s = eq_terms<TM2>(in_0);  for a = 1 .. n_rx - 1: eq_add<TM2>(s, in_a);  eq_finish<TM2>(s, noise, &x0, &x1);
// The inputs of one demap unit at one antenna: TM1 an RE (r0, h00); TM2 an SFBC RE pair (ra, rb) with the estimates
// h[port][RE] = h00 h01 / h10 h11
struct EqIn {
  float2 r0, r1, h00, h01, h10, h11;
};
// the running sums (named scalars, no arrays: they must stay in registers)
template <bool TM2>
struct EqAcc;
template <>
struct EqAcc<false> {
  float nx, ny, den;   // numerator re / im, sum |h|^2
};
template <>
struct EqAcc<true> {
  float hh, ax, ay, bx, by;   // sum (|h00|^2 + |h11|^2), x0 re / im and x1 re / im before the scaling
};
template <bool TM2>
__device__ __forceinline__ EqAcc<TM2> eq_terms(const EqIn& d) {
  MI_FP_EXACT
  EqAcc<TM2> t;
  if constexpr (!TM2) {
    const float2 y = d.r0, h = d.h00;
    t.nx = y.x * h.x + y.y * h.y;
    t.ny = y.y * h.x - y.x * h.y;
    t.den = h.x * h.x + h.y * h.y;
  } else {
    const float2 r0 = d.r0, r1 = d.r1, h00 = d.h00, h01 = d.h01, h10 = d.h10, h11 = d.h11;
    t.hh = h00.x * h00.x + h00.y * h00.y + h11.x * h11.x + h11.y * h11.y;
    t.ax = (h00.x * r0.x + h00.y * r0.y) + (h11.x * r1.x + h11.y * r1.y);
    t.ay = (h00.x * r0.y - h00.y * r0.x) + (h11.y * r1.x - h11.x * r1.y);
    t.bx = -(h10.x * r0.x + h10.y * r0.y) + (h01.x * r1.x + h01.y * r1.y);
    t.by = -(h10.y * r0.x - h10.x * r0.y) + (h01.x * r1.y - h01.y * r1.x);
  }
  return t;
}
template <bool TM2>
__device__ __forceinline__ void eq_add(EqAcc<TM2>& s, const EqIn& d) {
  MI_FP_EXACT
  const EqAcc<TM2> t = eq_terms<TM2>(d);
  if constexpr (!TM2) {
    s.nx = s.nx + t.nx;
    s.ny = s.ny + t.ny;
    s.den = s.den + t.den;
  } else {
    s.hh = s.hh + t.hh;
    s.ax = s.ax + t.ax;
    s.ay = s.ay + t.ay;
    s.bx = s.bx + t.bx;
    s.by = s.by + t.by;
  }
}
template <bool TM2>
__device__ __forceinline__ void eq_finish(const EqAcc<TM2>& s, float noise, float2* x0, float2* x1 /* TM2 only */) {
  MI_FP_EXACT
  if constexpr (!TM2) {
    const float den = s.den + noise;
    *x0 = make_float2(s.nx / den, s.ny / den);
  } else {
    float hh = s.hh;
    if (hh <= 0.f) hh = 1e-9f;
    const float sc = 1.41421356237309504880f / hh;
    *x0 = make_float2(sc * s.ax, sc * s.ay);
    *x1 = make_float2(sc * s.bx, sc * s.by);
  }
}

template <int QM>
__device__ __forceinline__ float pam_level(int lab) {
  // lab: this dimension's bits, MSB first (36.211 7.1 Gray mapping, separable I/Q)
  if constexpr (QM == 2) {
    return (1 - 2 * (lab & 1)) * 0.70710678118654752440f;
  } else if constexpr (QM == 4) {
    const int b0 = (lab >> 1) & 1, b1 = lab & 1;
    return (float)((1 - 2 * b0) * (1 + 2 * b1)) * 0.31622776601683793320f;
  } else {
    const int b0 = (lab >> 2) & 1, b1 = (lab >> 1) & 1, b2 = lab & 1;
    return (float)((1 - 2 * b0) * (4 - (1 - 2 * b1) * (2 - (1 - 2 * b2)))) * 0.15430334996209191026f;
  }
}

// writes the QM/2 LLRs of one dimension at llr[0], llr[2], llr[4] (I at even, Q at odd slots)
template <int QM>
__device__ __forceinline__ void demap_dim(float x, float* llr) {
  MI_FP_EXACT
  constexpr int NB = QM / 2, NL = 1 << NB;
  float d2[NL];
#pragma unroll
  for (int lab = 0; lab < NL; lab++) {
    const float d = x - pam_level<QM>(lab);
    d2[lab] = d * d;
  }
#pragma unroll
  for (int j = 0; j < NB; j++) {
    float m0 = 3.0e38f, m1 = 3.0e38f;
#pragma unroll
    for (int lab = 0; lab < NL; lab++) {
      if ((lab >> (NB - 1 - j)) & 1) m1 = fminf(m1, d2[lab]); else m0 = fminf(m0, d2[lab]);
    }
    llr[2 * j] = (m0 - m1) * 2.0f;   // / sigma^2, sigma^2 = 0.5
  }
}

// the QM LLRs of one equalised symbol, descrambled (scr bit bit0 + b set: sign flipped), to out[bit0 ..] as float2
// stores (QM and bit0 are even, the stream's base is 16-B aligned)
template <int QM>
__device__ __forceinline__ void demap_store(float2 x, const uint32_t* __restrict__ scr, uint32_t bit0,
                                            float* __restrict__ out) {
  float l[QM];
  demap_dim<QM>(x.x, l);
  demap_dim<QM>(x.y, l + 1);
#pragma unroll
  for (int b = 0; b < QM; b++) {
    const uint32_t i = bit0 + b;
    if ((scr[i >> 5] >> (i & 31)) & 1u) l[b] = -l[b];
  }
  float2* o = reinterpret_cast<float2*>(out + bit0);
#pragma unroll
  for (int b = 0; b < QM; b += 2) o[b / 2] = make_float2(l[b], l[b + 1]);
}

// LLR of bit j (MSB first) of one dimension: demap_dim's arithmetic for that bit alone (no dynamic
// register-array index)
template <int QM>
__device__ __forceinline__ float demap_bit(float x, uint32_t j) {
  MI_FP_EXACT
  constexpr int NB = QM / 2, NL = 1 << NB;
  float d2[NL];
#pragma unroll
  for (int lab = 0; lab < NL; lab++) {
    const float d = x - pam_level<QM>(lab);
    d2[lab] = d * d;
  }
  float out = 0.0f;
#pragma unroll
  for (int jj = 0; jj < NB; jj++) {
    float m0 = 3.0e38f, m1 = 3.0e38f;
#pragma unroll
    for (int lab = 0; lab < NL; lab++) {
      if ((lab >> (NB - 1 - jj)) & 1) m1 = fminf(m1, d2[lab]); else m0 = fminf(m0, d2[lab]);
    }
    out = (uint32_t)jj == j ? (m0 - m1) * 2.0f : out;
  }
  return out;
}

// one LLR of a PDSCH subframe: bit `gi` of the subframe's LLR stream (after descrambling), computed
// from the grids and channel estimates of the NRX antennas (antenna a's at g + a g_rx, c0 + a c_rx, c1 + a c_rx)
// exactly as demap_kernel computes it (TM1: one RE per Qm bits; TM2: one SFBC RE pair per 2 Qm bits)
template <int QM, int NRX>
__device__ __forceinline__ float demap_llr(const MiPdschDesc& pd, uint32_t gi, const float2* __restrict__ g,
                                           const float2* __restrict__ c0, const float2* __restrict__ c1,
                                           const uint32_t* __restrict__ re, const uint32_t* __restrict__ scr,
                                           float noise, size_t g_rx, size_t c_rx) {
  const uint32_t s = gi / QM, b = gi - s * QM;   // data symbol, bit within it
  float2 x;
  if constexpr (NRX == 1) {
    // one antenna: the loads as direct arguments, as before receive diversity (through a loader the compiler schedules
    // this path differently inside the rate de-matching combine loop, which runs at its register budget: rm.hip)
    if (pd.tm != 2) {
      const uint32_t r = re[s];
      x = eq_single(g[r], c0[r], noise);
    } else {
      const uint32_t u = s >> 1, ra = re[2 * u], rb = re[2 * u + 1];
      float2 x0, x1;
      eq_sfbc(g[ra], g[rb], c0[ra], c0[rb], c1[ra], c1[rb], &x0, &x1);
      x = (s & 1) == 0 ? x0 : x1;
    }
  } else if (pd.tm != 2) {
    const uint32_t r = re[s];
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
    eq_finish<false>(acc, noise, &x, nullptr);
  } else {
    const uint32_t u = s >> 1, ra = re[2 * u], rb = re[2 * u + 1];
    float2 x0, x1;
    EqAcc<true> acc = eq_terms<true>(EqIn{g[ra], g[rb], c0[ra], c0[rb], c1[ra], c1[rb]});
#pragma unroll
    for (int a = 1; a < NRX; a++) {
      const float2 *ga = g + a * g_rx, *p0 = c0 + a * c_rx, *p1 = c1 + a * c_rx;
      eq_add<true>(acc, EqIn{ga[ra], ga[rb], p0[ra], p0[rb], p1[ra], p1[rb]});
    }
    eq_finish<true>(acc, noise, &x0, &x1);
    x = (s & 1) == 0 ? x0 : x1;
  }
  const float v = demap_bit<QM>((b & 1) ? x.y : x.x, b >> 1);   // I: even bits, Q: odd bits
  return ((scr[gi >> 5] >> (gi & 31)) & 1u) ? -v : v;
}

}  // namespace mi
