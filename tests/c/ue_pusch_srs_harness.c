/*
 * ue_pusch_srs_harness.c -- drives the PUSCH calls of include/srslte/srslte.h in SRS subframes the way srsUE's
 * phch_worker drives them (phch_worker.cc:551-568): init_cell as for PUSCH (srslte_ue_ul_init, _set_rnti, _set_cfg
 * with the SRS, UCI and power-control configurations) plus mi_ue_ul_set_pusch_srs(rule), then per TTI
 * srslte_ue_ul_cfg_grant, srslte_ue_ul_pusch_encode_rnti_softbuffer and mi_ue_ul_pusch_power.
 * Input file : int32 hdr[20] = {cell_id, nof_prb, ncalls, group_hopping, sequence_hopping, delta_ss, rule, srs
 *              configured, subframe_config, bw_cfg, I_srs, B, b_hop, n_rrc, k_tc, n_srs (cyclic shift), rnti,
 *              delta_mcs_based, I_offset_ack, unused} + float f[16] = {unused, pathloss, p0_nominal_pusch, alpha,
 *              p0_nominal_pucch, delta_f_pucch[5], delta_preamble_msg3, p0_ue_pusch, p0_ue_pucch, p_srs_offset, unused,
 *              unused}; per call int32 c[12] = {tti, n_prb slot 0, n_prb slot 1, L_prb, tbs, Qm, rv, with data (0: NULL,
 *              the TB comes from the HARQ softbuffer), ack_len, ack, payload seed, unused}.  Payload byte i of seed s is
 *              (uint8_t)(131 s + 37 i + 11).  Different PRBs in the two slots go in as a type-1 hopping grant
 *              (hopping offset 0, intra-subframe mode), so cfg_grant sees them as its final per-slot PRBs.
 * Output file: per call int32 {ret of cfg_grant, ret of pusch_encode, mi_ue_ul_last_pusch_n_srs, grant.nof_symb} +
 *              float mi_ue_ul_pusch_power(PL, 0) + SF_LEN cf32 samples (zeros when a call failed).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi_ul.h"
#include "srslte/srslte.h"

#define MAX_TB_BYTES 4096

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  int32_t hdr[20];
  float f[16];
  if (fread(hdr, 4, 20, fi) != 20 || fread(f, 4, 16, fi) != 16) return 2;
  srslte_cell_t cell;
  memset(&cell, 0, sizeof(cell));
  cell.id = (uint32_t)hdr[0];
  cell.nof_prb = (uint32_t)hdr[1];
  cell.nof_ports = 1;
  cell.cp = SRSLTE_CP_NORM;
  srslte_ue_ul_t ue_ul;
  if (srslte_ue_ul_init(&ue_ul, cell)) { fprintf(stderr, "ue_ul_init\n"); return 3; }
  srslte_refsignal_dmrs_pusch_cfg_t dmrs_cfg;
  srslte_pusch_hopping_cfg_t pusch_hopping;
  srslte_refsignal_srs_cfg_t srs_cfg;
  srslte_pucch_cfg_t pucch_cfg;
  srslte_pucch_sched_t pucch_sched;
  srslte_uci_cfg_t uci_cfg;
  srslte_ue_ul_powerctrl_t power_ctrl;
  memset(&dmrs_cfg, 0, sizeof(dmrs_cfg)); memset(&pusch_hopping, 0, sizeof(pusch_hopping));
  memset(&srs_cfg, 0, sizeof(srs_cfg)); memset(&pucch_cfg, 0, sizeof(pucch_cfg));
  memset(&pucch_sched, 0, sizeof(pucch_sched)); memset(&uci_cfg, 0, sizeof(uci_cfg));
  memset(&power_ctrl, 0, sizeof(power_ctrl));
  dmrs_cfg.group_hopping_en = hdr[3] != 0;
  dmrs_cfg.sequence_hopping_en = hdr[4] != 0;
  dmrs_cfg.delta_ss = (uint32_t)hdr[5];
  srs_cfg.configured = hdr[7] != 0;
  srs_cfg.subframe_config = (uint32_t)hdr[8];
  srs_cfg.bw_cfg = (uint32_t)hdr[9];
  srs_cfg.I_srs = (uint32_t)hdr[10];
  srs_cfg.B = (uint32_t)hdr[11];
  srs_cfg.b_hop = (uint32_t)hdr[12];
  srs_cfg.n_rrc = (uint32_t)hdr[13];
  srs_cfg.k_tc = (uint32_t)hdr[14];
  srs_cfg.n_srs = (uint32_t)hdr[15];
  pucch_cfg.delta_pucch_shift = 1;
  pusch_hopping.n_sb = 1;
  uci_cfg.I_offset_ack = (uint32_t)hdr[18];
  uci_cfg.I_offset_cqi = 2;
  power_ctrl.p0_nominal_pusch = f[2];
  power_ctrl.alpha = f[3];
  power_ctrl.p0_nominal_pucch = f[4];
  for (int i = 0; i < 5; i++) power_ctrl.delta_f_pucch[i] = f[5 + i];
  power_ctrl.delta_preamble_msg3 = f[10];
  power_ctrl.p0_ue_pusch = f[11];
  power_ctrl.p0_ue_pucch = f[12];
  power_ctrl.p_srs_offset = f[13];
  power_ctrl.delta_mcs_based = hdr[17] != 0;
  srslte_ue_ul_set_cfg(&ue_ul, &dmrs_cfg, &srs_cfg, &pucch_cfg, &pucch_sched, &uci_cfg, &pusch_hopping, &power_ctrl);
  srslte_ue_ul_set_rnti(&ue_ul, (uint16_t)hdr[16]);
  mi_ue_ul_set_pusch_srs(&ue_ul, (uint32_t)hdr[6]);
  srslte_softbuffer_tx_t softbuffer;
  if (srslte_softbuffer_tx_init(&softbuffer, 100)) { fprintf(stderr, "softbuffer_tx\n"); return 3; }
  const uint32_t sflen = SRSLTE_SF_LEN_PRB(cell.nof_prb);
  cf_t *signal = (cf_t *)srslte_vec_malloc(sflen * sizeof(cf_t));
  static uint8_t payload[MAX_TB_BYTES];
  for (int i = 0; i < hdr[2]; i++) {
    int32_t c[12];
    if (fread(c, 4, 12, fi) != 12) return 4;
    if (c[4] <= 0 || c[4] / 8 > MAX_TB_BYTES) return 4;
    srslte_ra_ul_grant_t grant;
    srslte_uci_data_t uci_data;
    memset(&grant, 0, sizeof(grant));
    memset(&uci_data, 0, sizeof(uci_data));
    grant.n_prb[0] = grant.n_prb_tilde[0] = (uint32_t)c[1];
    grant.n_prb[1] = grant.n_prb_tilde[1] = (uint32_t)c[2];
    grant.freq_hopping = c[1] != c[2] ? 1 : 0;
    grant.L_prb = (uint32_t)c[3];
    grant.nof_symb = 12;
    grant.nof_re = 12 * 12 * grant.L_prb;
    grant.mcs.tbs = c[4];
    grant.Qm = (uint32_t)c[5];
    uci_data.uci_ack_len = (uint32_t)c[8];
    uci_data.uci_ack = (uint8_t)c[9];
    for (int k = 0; k < c[4] / 8; k++) payload[k] = (uint8_t)(131 * c[10] + 37 * k + 11);
    memset(signal, 0, sflen * sizeof(cf_t));
    int32_t out[4] = {0, 0, 0, 0};
    out[0] = srslte_ue_ul_cfg_grant(&ue_ul, &grant, (uint32_t)c[0], (uint32_t)c[6], 0);
    if (!out[0])
      out[1] = srslte_ue_ul_pusch_encode_rnti_softbuffer(&ue_ul, c[7] ? payload : NULL, uci_data, &softbuffer,
                                                         (uint16_t)hdr[16], signal);
    else
      out[1] = -100;
    out[2] = (int32_t)mi_ue_ul_last_pusch_n_srs(&ue_ul);
    out[3] = (int32_t)ue_ul.pusch_cfg.grant.nof_symb;
    const float tx_power = mi_ue_ul_pusch_power(&ue_ul, f[1], 0.0f);
    fwrite(out, 4, 4, fo);
    fwrite(&tx_power, 4, 1, fo);
    fwrite(signal, 8, sflen, fo);
  }
  srslte_softbuffer_tx_free(&softbuffer);
  srslte_ue_ul_free(&ue_ul);
  srslte_vec_free(signal);
  fclose(fi);
  fclose(fo);
  return 0;
}
