// srs_host.cpp -- host planner of the SRS transmitter (see srs.h; no HIP calls).  Spec arithmetic: 36.211 5.5.3.1
// (sequence), 5.5.3.2 (bandwidth tables, frequency position and hopping), 5.5.1.3 / 5.5.1.4 (group and sequence
// hopping), 36.213 8.2 (periodicity).  DESIGN.md carries the formulas as implemented.
#include "srs.h"

#include "plan.h"     // set_error
#include "ul_plan.h"  // ul_base_seq, ul_group_u, ul_seq_hop_bit

namespace mi {
namespace {

// 36.211 Tables 5.5.3.2-1 .. 5.5.3.2-4: m_SRS,b for [table][b][C_SRS]; N_b = m_SRS,b-1 / m_SRS,b is derived
const uint8_t M_SRS[4][4][8] = {
    {{36, 32, 24, 20, 16, 12, 8, 4}, {12, 16, 4, 4, 4, 4, 4, 4}, {4, 8, 4, 4, 4, 4, 4, 4}, {4, 4, 4, 4, 4, 4, 4, 4}},
    {{48, 48, 40, 36, 32, 24, 20, 16}, {24, 16, 20, 12, 16, 4, 4, 4}, {12, 8, 4, 4, 8, 4, 4, 4}, {4, 4, 4, 4, 4, 4, 4, 4}},
    {{72, 64, 60, 48, 48, 40, 36, 32}, {24, 32, 20, 24, 16, 20, 12, 16}, {12, 16, 4, 12, 8, 4, 4, 8}, {4, 4, 4, 4, 4, 4, 4, 4}},
    {{96, 96, 80, 72, 64, 60, 48, 48}, {48, 32, 40, 24, 32, 20, 24, 16}, {24, 16, 20, 12, 16, 4, 12, 8}, {4, 4, 4, 4, 4, 4, 4, 4}}};

uint32_t bw_table(uint32_t nof_prb) { return nof_prb <= 40 ? 0 : nof_prb <= 60 ? 1 : nof_prb <= 80 ? 2 : 3; }

// every field of c; false + set_error
bool check(const mi_srs_cfg_t& c) {
  if (!std_nof_prb(c.nof_prb)) {
    set_error("SRS: nof_prb must be one of 6, 15, 25, 50, 75, 100");
    return false;
  }
  if (c.cell_id > 503 || c.tti > 10239) {
    set_error("SRS: cell_id 0..503, tti 0..10239");
    return false;
  }
  if (c.bw_cfg > 7 || c.B > 3 || c.b_hop > 3 || c.n_rrc > 23 || c.k_tc > 1 || c.n_srs > 7) {
    set_error("SRS: bw_cfg 0..7, B 0..3, b_hop 0..3, n_rrc 0..23, k_tc 0..1, n_srs (cyclic shift) 0..7");
    return false;
  }
  uint32_t T, off;
  if (srs_ue_period(c.I_srs, &T, &off)) {
    set_error("SRS: I_srs 637..1023 is reserved (36.213 Table 8.2-1)");
    return false;
  }
  if (c.delta_ss > 29) {
    set_error("SRS: delta_ss 0..29");
    return false;
  }
  if (M_SRS[bw_table(c.nof_prb)][0][c.bw_cfg] > c.nof_prb) {
    set_error("SRS: m_SRS,0 of this bw_cfg exceeds nof_prb");
    return false;
  }
  return true;
}

void derive(const mi_srs_cfg_t& c, mi_srs_res_t* r) {
  uint32_t m[4], Nb[4], T, off;
  for (uint32_t b = 0; b < 4; b++) {
    m[b] = M_SRS[bw_table(c.nof_prb)][b][c.bw_cfg];
    Nb[b] = b ? m[b - 1] / m[b] : 1;
  }
  srs_ue_period(c.I_srs, &T, &off);
  const uint32_t n_SRS = c.tti / T;   // FDD: floor((10 n_f + floor(n_s / 2)) / T_SRS)
  uint32_t k0 = (c.nof_prb / 2 - m[0] / 2) * 12 + c.k_tc;
  // prev = prod_{b' = b_hop .. b - 1} N_b' with N_b_hop taken as 1 (5.5.3.2)
  uint32_t prev = 1;
  for (uint32_t b = 0; b < 4; b++) {
    uint32_t nb = 0;
    if (b <= c.B) {
      nb = 4 * c.n_rrc / m[b];
      if (c.b_hop < c.B && b > c.b_hop) {
        const uint32_t cur = prev * Nb[b];
        const uint32_t F = Nb[b] % 2 == 0 ? (Nb[b] / 2) * ((n_SRS % cur) / prev) + (n_SRS % cur) / (2 * prev)
                                          : (Nb[b] / 2) * (n_SRS / prev);
        nb += F;
        prev = cur;
      }
      nb %= Nb[b];
      k0 += 12 * m[b] * nb;
    }
    r->n_b[b] = nb;
  }
  r->m_srs = m[c.B];
  r->M_sc = 6 * m[c.B];
  r->k0 = k0;
  r->n_SRS = n_SRS;
  r->T_srs = T;
  // 5.5.1.3: the PUCCH sequence-shift pattern f_ss = N_ID mod 30; 5.5.1.4: c_init uses the PUSCH one
  const uint32_t ns = 2 * (c.tti % 10) + 1;
  r->u = ul_group_u(c.cell_id, ns, c.group_hopping, c.cell_id % 30);
  r->v = 0;
  if (c.sequence_hopping && !c.group_hopping && r->M_sc >= 72)
    r->v = ul_seq_hop_bit(c.cell_id, (c.cell_id % 30 + c.delta_ss) % 30, ns);
  ul_base_seq(r->M_sc, r->u, r->v, &r->q, &r->nzc);
  r->n_cs = c.n_srs;
}

}  // namespace

int SrsPlan::build(const mi_srs_cfg_t* cfgs, uint32_t n) {
  txs.clear();
  res.clear();
  iq_samples = 0;
  for (uint32_t i = 0; i < n; i++)
    if (!check(cfgs[i])) return -1;
  for (uint32_t i = 0; i < n; i++) {
    const mi_srs_cfg_t& c = cfgs[i];
    mi_srs_res_t r;
    derive(c, &r);
    MiSrsTx t{};
    t.N = (uint32_t)symbol_sz(c.nof_prb);
    t.M_sc = r.M_sc;
    t.K = (int32_t)r.k0 - 6 * (int32_t)c.nof_prb;
    t.nzc = r.nzc;
    t.q = r.q;
    t.n_cs = r.n_cs;
    t.scale = 1.0f;
    t.cfo = 0.0f;
    t.iq_off = iq_samples;
    iq_samples += 15 * (size_t)t.N;
    txs.push_back(t);
    res.push_back(r);
  }
  return 0;
}

}  // namespace mi

extern "C" {

uint32_t mi_srs_resource_n(const mi_srs_cfg_t* c, uint32_t n, mi_srs_res_t* r) {
  if (!c || !r) { mi::set_error("SRS: null argument"); return 0; }
  for (uint32_t i = 0; i < n; i++) {
    if (!mi::check(c[i])) return i;
    mi::derive(c[i], &r[i]);
  }
  return n;
}

int mi_srs_resource(const mi_srs_cfg_t* c, mi_srs_res_t* r) { return mi_srs_resource_n(c, 1, r) == 1 ? 0 : -1; }

int srslte_refsignal_srs_send_cs(uint32_t subframe_config, uint32_t sf_idx);   // srslte_util.cpp (srslte/srslte.h)

// 36.211 5.3.4: the PUSCH leaves the last symbol of a subframe in which the UE sends its SRS, and of a cell-specific
// SRS subframe when its PRBs meet the cell's sounding band (the m_SRS,0 PRBs centred in the carrier, 5.5.3.2)
int mi_ul_pusch_n_srs(uint32_t nof_prb, uint32_t srs_subframe_config, uint32_t srs_bw_cfg, uint32_t sf_idx, uint32_t n_prb0,
                      uint32_t n_prb1, uint32_t L_prb, int ue_sends_srs, uint32_t rule) {
  if (!mi::std_nof_prb(nof_prb) || srs_subframe_config > 14 || srs_bw_cfg > 7 || sf_idx > 9 || L_prb < 1 ||
      n_prb0 + L_prb > nof_prb || n_prb1 + L_prb > nof_prb || rule > MI_PUSCH_SRS_ALL_CS)
    return -1;
  const uint32_t m0 = mi::M_SRS[mi::bw_table(nof_prb)][0][srs_bw_cfg];
  if (m0 > nof_prb) return -1;
  if (rule == MI_PUSCH_SRS_OFF) return 0;
  if (ue_sends_srs) return 1;
  if (srslte_refsignal_srs_send_cs(srs_subframe_config, sf_idx) != 1) return 0;
  if (rule == MI_PUSCH_SRS_ALL_CS) return 1;
  const uint32_t lo = nof_prb / 2 - m0 / 2, hi = lo + m0;   // the band is PRBs lo .. hi - 1
  auto meets = [&](uint32_t p) { return p < hi && p + L_prb > lo; };
  return meets(n_prb0) || meets(n_prb1) ? 1 : 0;
}

}  // extern "C"
