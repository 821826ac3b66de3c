// csi_body.h -- CSI feedback (CQI / PMI / RI) from the channel estimates: the arithmetic of csi_kernel (csi.hip),
// shared with the host emulation (emu.cpp emu_csi).  Definitions: include/mi_dl.h, DESIGN.md 10.
//
// A sample point (one subcarrier of one CRS symbol) holds H[a][p] = antenna a's estimate of port p.  With
//   P0 = sum_a |h_a0|^2,  P1 = sum_a |h_a1|^2,  S = P0 + P1,  C = sum_a h_a0* h_a1,  D = |h_00 h_11 - h_01 h_10|^2
// every hypothesis follows without forming a matrix:
//   rank 1, q:   sum_a |h_a0 + q h_a1|^2 = S + 2 Re(q C)                       (q = 1, -1, j, -j: Cr, -Cr, -Ci, Ci)
//   rank 2, w:   A = I + G^H G / n = [[a, b], [b*, d]],  a, d = 1 + (S +- 2 Re(w C)) / (4 n)    (w = 1: Cr, w = j: -Ci)
//                det A = 1 + tr + det = 1 + S / (2 n) + D / (4 n^2)   (|det P| = 1/2: the same for both w, and free of
//                the cancellation of a d - |b|^2 on a rank-deficient channel)
//                1 + g_0 = det A / d,  1 + g_1 = det A / a
// so log2(1 + g_l) = log2 det A - log2 d (or a): the point accumulates log2 det A once and log2 a, log2 d per w --
// ten logarithms, no division -- and the capacities are differences of the reduced sums.
#pragma once
#include "cqi_table.h"
#include "demap_body.h"
#include "mi_dl.h"

struct MiCsiSf {             // one per physical subframe (an entry that owns samples) of the batch
  uint64_t ce_off;           // float2 offset of its port-0 channel estimates (antenna 0)
  uint32_t W, ports;
  uint32_t sb_prb, n_sb;     // subbands (36.213 Table 7.2.1-3); 0, 0 = none
  uint32_t sf;               // its entry index: metrics row, noise value and record
  uint32_t dup;              // the cw = 1 entry that reports the same record, 0xFFFFFFFF = none
};

namespace mi {

// the reduced sums of a band: log2(1 + g) of BASE and of the four rank-1 precoders, then log2 det A and log2 a, log2 d
// of w = 1 and w = j
enum { CSI_BASE = 0, CSI_R1 = 1, CSI_DET = 5, CSI_A1 = 6, CSI_D1 = 7, CSI_AJ = 8, CSI_DJ = 9, CSI_NACC = 10 };
constexpr int CSI_CELLS = (1 + MI_CSI_MAX_SB) * MI_CSI_NHYP * 2;

// 36.213 Table 7.2.1-3 (higher-layer-configured subbands); false for a bandwidth outside 6..110 PRB
__host__ __device__ inline bool csi_subbands(uint32_t nof_prb, uint32_t* sb_prb, uint32_t* n_sb) {
  if (nof_prb < 6 || nof_prb > (uint32_t)NRB_MAX) return false;
  const uint32_t k = nof_prb <= 7 ? 0u : nof_prb <= 26 ? 4u : nof_prb <= 63 ? 6u : 8u;
  *sb_prb = k;
  *n_sb = k ? (nof_prb + k - 1) / k : 0u;
  return true;
}

__host__ __device__ inline uint32_t csi_valid_mask(uint32_t ports, uint32_t n_rx) {
  return ports < 2 ? 1u : n_rx < 2 ? 0x1Fu : 0xFFu;
}

// One point into the band's ten accumulators.  Absent estimates (a second port or antenna the batch does not have)
// are passed as zeros; mask = csi_valid_mask, uniform over a workgroup.
__device__ __forceinline__ void csi_point(float2 h00, float2 h01, float2 h10, float2 h11, uint32_t mask, float inv_n,
                                          float* acc) {
  const float p0 = (h00.x * h00.x + h00.y * h00.y) + (h10.x * h10.x + h10.y * h10.y);
  if (!(mask & 2u)) {   // one port
    acc[CSI_BASE] += log2f(1.0f + p0 * inv_n);
    return;
  }
  const float p1 = (h01.x * h01.x + h01.y * h01.y) + (h11.x * h11.x + h11.y * h11.y);
  const float s = p0 + p1;
  const float cr = (h00.x * h01.x + h00.y * h01.y) + (h10.x * h11.x + h10.y * h11.y);   // C = sum_a h_a0* h_a1
  const float ci = (h00.x * h01.y - h00.y * h01.x) + (h10.x * h11.y - h10.y * h11.x);
  const float hn = 0.5f * inv_n;
  acc[CSI_BASE] += log2f(1.0f + s * hn);
  // a sum of squares: never below 0 but for rounding
  acc[CSI_R1 + 0] += log2f(1.0f + fmaxf(s + 2.0f * cr, 0.0f) * hn);
  acc[CSI_R1 + 1] += log2f(1.0f + fmaxf(s - 2.0f * cr, 0.0f) * hn);
  acc[CSI_R1 + 2] += log2f(1.0f + fmaxf(s - 2.0f * ci, 0.0f) * hn);
  acc[CSI_R1 + 3] += log2f(1.0f + fmaxf(s + 2.0f * ci, 0.0f) * hn);
  if (!(mask & (1u << MI_CSI_H_R2))) return;
  const float dx = (h00.x * h11.x - h00.y * h11.y) - (h01.x * h10.x - h01.y * h10.y);   // det H
  const float dy = (h00.x * h11.y + h00.y * h11.x) - (h01.x * h10.y + h01.y * h10.x);
  const float qn = 0.25f * inv_n;
  acc[CSI_DET] += log2f(1.0f + s * hn + (dx * dx + dy * dy) * (qn * inv_n));
  acc[CSI_A1] += log2f(1.0f + fmaxf(s + 2.0f * cr, 0.0f) * qn);
  acc[CSI_D1] += log2f(1.0f + fmaxf(s - 2.0f * cr, 0.0f) * qn);
  acc[CSI_AJ] += log2f(1.0f + fmaxf(s - 2.0f * ci, 0.0f) * qn);
  acc[CSI_DJ] += log2f(1.0f + fmaxf(s + 2.0f * ci, 0.0f) * qn);
}

// cap[.][h][layer] of a band from its sums s and 1 / (its number of points); 0 where the hypothesis is not evaluated
__host__ __device__ inline float csi_cap(const float* s, float inv_cnt, uint32_t h, uint32_t layer, uint32_t mask) {
  if (!((mask >> h) & 1u)) return 0.0f;
  if (h < (uint32_t)MI_CSI_H_CDD) return layer ? 0.0f : s[h] * inv_cnt;
  // rounding may leave a vanishing layer's difference of sums just below 0
  const float c0 = fmaxf(s[CSI_DET] - s[h == 7 ? CSI_DJ : CSI_D1], 0.0f) * inv_cnt;
  const float c1 = fmaxf(s[CSI_DET] - s[h == 7 ? CSI_AJ : CSI_A1], 0.0f) * inv_cnt;
  if (h == (uint32_t)MI_CSI_H_CDD) return 0.5f * (c0 + c1);   // w = -1 is w = +1 with its layers swapped
  return layer ? c1 : c0;
}

// the CQI of a capacity: srslte_cqi_from_snr of the SINR (dB) that alone gives it
__host__ __device__ inline uint8_t csi_cqi(float cap) {
  return cap > 0.0f ? cqi_from_snr_db(10.0f * log10f(exp2f(cap) - 1.0f)) : (uint8_t)0;
}

// points of band `band` (0 = the whole bandwidth) of a cell of nof_prb = W / 12
__host__ __device__ inline uint32_t csi_band_points(uint32_t band, uint32_t W, uint32_t sb_prb, uint32_t n_sb) {
  if (band == 0) return 4u * W;
  return 4u * (band < n_sb ? 12u * sb_prb : W - (n_sb - 1u) * 12u * sb_prb);
}

// Cell t (= (band * MI_CSI_NHYP + h) * 2 + layer) of the record from the band sums: sums[0] = the whole bandwidth,
// sums[1 + c] = subband c
__device__ __forceinline__ void csi_cell(uint32_t t, const float (*sums)[CSI_NACC], const MiCsiSf& d, uint32_t mask,
                                         mi_dl_csi_result_t* out) {
  const uint32_t band = t / (2u * MI_CSI_NHYP), h = (t >> 1) % MI_CSI_NHYP, layer = t & 1u;
  float c = 0.0f;
  if (band <= d.n_sb) c = csi_cap(sums[band], 1.0f / (float)csi_band_points(band, d.W, d.sb_prb, d.n_sb), h, layer, mask);
  out->cap[band][h][layer] = c;
  out->cqi[band][h][layer] = csi_cqi(c);
}

// the record's scalars: the decisions from the wideband capacities (ties to the lower index)
__device__ __forceinline__ void csi_decide(const float* wide, const MiCsiSf& d, uint32_t mask, float noise,
                                           mi_dl_csi_result_t* out) {
  const float inv = 1.0f / (float)(4u * d.W);
  uint32_t pmi = 0, cb = 0, ri_cl = 1, ri_ol = 1;
  if (mask & 2u) {
    float best = csi_cap(wide, inv, MI_CSI_H_R1, 0, mask);
    for (uint32_t i = 1; i < 4; i++) {
      const float c = csi_cap(wide, inv, MI_CSI_H_R1 + i, 0, mask);
      if (c > best) { best = c; pmi = i; }
    }
    if (mask & (1u << MI_CSI_H_R2)) {
      const float r1 = csi_cap(wide, inv, MI_CSI_H_R2, 0, mask) + csi_cap(wide, inv, MI_CSI_H_R2, 1, mask);
      const float rj = csi_cap(wide, inv, MI_CSI_H_R2 + 1, 0, mask) + csi_cap(wide, inv, MI_CSI_H_R2 + 1, 1, mask);
      cb = rj > r1 ? 2u : 1u;
      if (fmaxf(r1, rj) > best) ri_cl = 2;
      if (2.0f * csi_cap(wide, inv, MI_CSI_H_CDD, 0, mask) > csi_cap(wide, inv, MI_CSI_H_BASE, 0, mask)) ri_ol = 2;
    }
  }
  out->valid_mask = mask;
  out->n_sb = d.n_sb;
  out->sb_prb = d.sb_prb;
  out->pmi_r1 = pmi;
  out->cb_r2 = cb;
  out->ri_cl = ri_cl;
  out->ri_ol = ri_ol;
  out->noise = noise;
}

}  // namespace mi
