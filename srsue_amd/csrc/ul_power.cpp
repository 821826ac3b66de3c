// ul_power.cpp -- open-loop UL power control (36.213 5.1.1.1 PUSCH, 5.1.2.1 PUCCH, 5.1.3.1 SRS), host only (no HIP
// calls): what srsUE asks for after each transmission (srsUE phch_worker.cc:568, :622, :652).  The TPC accumulations
// f(i) and g(i) are 0: acc_enabled is stored and unused.  DESIGN.md carries the formulas as implemented.
#include <math.h>

#include "mi_ul.h"

namespace {
// the terms are added in double precision, so that the float result is the rounded closed form
float cap(double p) { return (float)(p < (double)MI_UL_P_CMAX ? p : (double)MI_UL_P_CMAX); }
}  // namespace

extern "C" {

float mi_ul_pusch_power(const mi_ul_power_cfg_t* p, float PL, float p0_preamble, uint32_t L_prb, uint32_t sum_Kr) {
  return mi_ul_pusch_power_nsymb(p, PL, p0_preamble, L_prb, sum_Kr, 12);
}

float mi_ul_pusch_power_nsymb(const mi_ul_power_cfg_t* p, float PL, float p0_preamble, uint32_t L_prb, uint32_t sum_Kr,
                              uint32_t n_symb_initial) {
  if (!p || !L_prb || !n_symb_initial) return 0.0f;
  // a grant of the random-access response: j = 2, P0 = P0_PRE + Delta_PREAMBLE_Msg3, alpha = 1
  const bool msg3 = p0_preamble != 0.0f;
  const double p0 = msg3 ? (double)p0_preamble + p->delta_preamble_msg3 : (double)p->p0_nominal_pusch + p->p0_ue_pusch;
  const double alpha = msg3 ? 1.0 : p->alpha;
  double delta_tf = 0.0;
  if (p->delta_mcs_based) {   // K_S = 1.25, beta_offset^PUSCH = 1 (data is sent); N_RE = M_sc^PUSCH N_symb^PUSCH-initial
    const double bpre = (double)sum_Kr / (12.0 * (double)n_symb_initial * (double)L_prb);
    delta_tf = 10.0 * log10(pow(2.0, 1.25 * bpre) - 1.0);
  }
  return cap(10.0 * log10((double)L_prb) + p0 + alpha * PL + delta_tf);
}

float mi_ul_pucch_power(const mi_ul_power_cfg_t* p, float PL, uint32_t format, uint32_t n_cqi, uint32_t /*n_harq*/) {
  if (!p) return 0.0f;
  // normal CP: h = 10 log10(n_CQI / 4) for formats 2/2a/2b with n_CQI >= 4, 0 for formats 1/1a/1b
  const double h = format >= MI_PUCCH_2 && format <= MI_PUCCH_2B && n_cqi >= 4 ? 10.0 * log10((double)n_cqi / 4.0) : 0.0;
  // deltaF-PUCCH: formats 1, 1b, 2, 2a, 2b; 1a is the reference format
  const double df = format == MI_PUCCH_1 ? p->delta_f_pucch[0]
                 : format == MI_PUCCH_1B ? p->delta_f_pucch[1]
                 : format >= MI_PUCCH_2 && format <= MI_PUCCH_2B ? p->delta_f_pucch[format - MI_PUCCH_2 + 2] : 0.0f;
  return cap((double)p->p0_nominal_pucch + p->p0_ue_pucch + PL + h + df);
}

float mi_ul_srs_power(const mi_ul_power_cfg_t* p, float PL, uint32_t m_srs) {
  if (!p || !m_srs) return 0.0f;
  const double off = p->delta_mcs_based ? -3.0 + p->p_srs_offset : -10.5 + 1.5 * p->p_srs_offset;
  return cap(off + 10.0 * log10((double)m_srs) + p->p0_nominal_pusch + p->p0_ue_pusch + (double)p->alpha * PL);
}

}  // extern "C"
