// sm_body.h -- two-layer spatial multiplexing detection (TM3 large-delay CDD, TM4 closed loop): the arithmetic of
// sm_detect_kernel (sm_detect.hip), shared with the host emulation (emu.cpp emu_pdsch_llr_sm) so that both give the
// same floats.  2 CRS ports, 2 receive antennas, 2 layers, one codeword per layer (36.211 6.3.3.2: x0(i) = d0(i),
// x1(i) = d1(i)).
//
// Precoding (36.211 6.3.4.2.2 / 6.3.4.2.3), [y_port0; y_port1] = P_i [x0; x1] at RE i of the PDSCH mapping order:
//   TM3          P_i = W D(i) U = (1/2) [[1, 1], [s, -s]],  s = (-1)^i
//   TM4 pmi 1    P_i = (1/2) [[1, 1], [1, -1]]
//   TM4 pmi 2    P_i = (1/2) [[1, 1], [j, -j]]
// i.e. P_i = (1/2) [[1, 1], [w, -w]] with w in {1, -1, j}.  With H[a][p] antenna a's estimate of port p the effective
// channel G = H P_i has the columns g_a0 = (h_a0 + w h_a1) / 2 (layer 0) and g_a1 = (h_a0 - w h_a1) / 2 (layer 1).
// Detector (a project convention, biased like eq_single, no per-layer SINR weighting):
//   x^ = (G^H G + noise I)^-1 G^H y, in its closed 2 x 2 form.
#pragma once
#include "demap_body.h"

namespace mi {

// w h for the precoder mode (MiSmDesc::mode) at RE index i
__device__ __forceinline__ float2 sm_rot(float2 h, uint32_t mode, uint32_t i) {
  if (mode == 2) return make_float2(-h.y, h.x);                 // j h
  if (mode == 0 && (i & 1u)) return make_float2(-h.x, -h.y);    // TM3, odd i: s = -1
  return h;
}

// y_a: antenna a's received RE; h_ap: antenna a's estimate of port p.  Named scalars, no arrays: they stay in registers.
__device__ __forceinline__ void sm_mmse(float2 y0, float2 y1, float2 h00, float2 h01, float2 h10, float2 h11,
                                       uint32_t mode, uint32_t i, float noise, float2* x0, float2* x1) {
  MI_FP_EXACT
  const float2 t0 = sm_rot(h01, mode, i), t1 = sm_rot(h11, mode, i);
  // g_al: antenna a, layer l
  const float g00x = 0.5f * (h00.x + t0.x), g00y = 0.5f * (h00.y + t0.y);
  const float g01x = 0.5f * (h00.x - t0.x), g01y = 0.5f * (h00.y - t0.y);
  const float g10x = 0.5f * (h10.x + t1.x), g10y = 0.5f * (h10.y + t1.y);
  const float g11x = 0.5f * (h10.x - t1.x), g11y = 0.5f * (h10.y - t1.y);
  // G^H G + noise I = [[a, b], [b*, d]]
  const float a = (g00x * g00x + g00y * g00y) + (g10x * g10x + g10y * g10y) + noise;
  const float d = (g01x * g01x + g01y * g01y) + (g11x * g11x + g11y * g11y) + noise;
  const float bx = (g00x * g01x + g00y * g01y) + (g10x * g11x + g10y * g11y);   // b = g00* g01 + g10* g11
  const float by = (g00x * g01y - g00y * g01x) + (g10x * g11y - g10y * g11x);
  // z = G^H y
  const float z0x = (g00x * y0.x + g00y * y0.y) + (g10x * y1.x + g10y * y1.y);
  const float z0y = (g00x * y0.y - g00y * y0.x) + (g10x * y1.y - g10y * y1.x);
  const float z1x = (g01x * y0.x + g01y * y0.y) + (g11x * y1.x + g11y * y1.y);
  const float z1y = (g01x * y0.y - g01y * y0.x) + (g11x * y1.y - g11y * y1.x);
  float det = a * d - (bx * bx + by * by);
  if (det <= 0.f) det = 1e-9f;
  // x0 = (d z0 - b z1) / det,  x1 = (a z1 - b* z0) / det
  *x0 = make_float2((d * z0x - (bx * z1x - by * z1y)) / det, (d * z0y - (bx * z1y + by * z1x)) / det);
  *x1 = make_float2((a * z1x - (bx * z0x + by * z0y)) / det, (a * z1y - (bx * z0y - by * z0x)) / det);
}

// RE i of a pair: gather (the RE list, as demap_kernel), detect once, then each codeword's Qm LLRs into its own stream
// (demap_store's float2 stores).  g / c: antenna 0's grid and port-0 estimates of the subframe; antenna 1's are g_rx /
// c_rx elements on, port 1's d.c1 on.
__device__ __forceinline__ void sm_detect_re(const MiSmDesc& d, uint32_t i, const float2* __restrict__ g,
                                            const float2* __restrict__ c, const uint32_t* __restrict__ re_tab,
                                            const uint32_t* __restrict__ scr_tab, float* __restrict__ e, float noise,
                                            size_t g_rx, size_t c_rx) {
  const uint32_t r = re_tab[d.re + i];
  float2 x0, x1;
  sm_mmse(g[r], g[g_rx + r], c[r], c[d.c1 + r], c[c_rx + r], c[c_rx + d.c1 + r], d.mode, i, noise, &x0, &x1);
  const uint32_t* s0 = scr_tab + d.scr0;
  const uint32_t* s1 = scr_tab + d.scr1;
  float* e0 = e + d.e0;
  float* e1 = e + d.e1;
  switch (d.qm0) {
    case 2: demap_store<2>(x0, s0, i * 2, e0); break;
    case 4: demap_store<4>(x0, s0, i * 4, e0); break;
    default: demap_store<6>(x0, s0, i * 6, e0); break;
  }
  switch (d.qm1) {
    case 2: demap_store<2>(x1, s1, i * 2, e1); break;
    case 4: demap_store<4>(x1, s1, i * 4, e1); break;
    default: demap_store<6>(x1, s1, i * 6, e1); break;
  }
}

}  // namespace mi
