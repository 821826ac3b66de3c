/*
 * ue_srs_harness.c -- drives mi_ue_ul_srs_encode and the mi_ue_ul_*_power calls (include/srslte/srslte.h) the way
 * srsUE's phch_worker drives its SRS encode and power calls (phch_worker.cc:636-656, :568, :622): init_cell as for
 * PUSCH (srslte_ue_ul_init, _set_normalization, _set_cfo_enable, _set_rnti, _set_cfg with the SRS and power-control
 * configurations), then per TTI srslte_ue_ul_set_cfo, mi_ue_ul_srs_encode(&ue_ul, tti, signal) and
 * mi_ue_ul_srs_power(&ue_ul, pathloss).
 * Input file : int32 hdr[20] = {cell_id, nof_prb, ncalls, group_hopping, sequence_hopping, delta_ss, flags (1 =
 *              normalisation, 2 = CFO), srs configured, subframe_config, bw_cfg, I_srs, B, b_hop, n_rrc, k_tc, n_srs,
 *              pusch, rnti, delta_mcs_based, acc_enabled} + float f[16] = {cfo, pathloss, p0_nominal_pusch, alpha,
 *              p0_nominal_pucch, delta_f_pucch[5], delta_preamble_msg3, p0_ue_pusch, p0_ue_pucch, p_srs_offset,
 *              p0_preamble, unused}; per call int32 tti.  pusch = 1: one PUSCH subframe (3 PRB, 256 bits, QPSK) is
 *              encoded before the SRS calls, and again after them from the HARQ softbuffer (payload NULL).
 * Output file: per call int32 ret + float srs_power + SF_LEN cf32 samples; then float pw[9] = {pusch_power(PL, 0),
 *              pusch_power(PL, p0_preamble), pucch_power(PL, format 0..5, n_cqi 11, n_harq 1), srs_power(PL)}; with
 *              pusch = 1 then int32 {ret before, ret after} + the two PUSCH subframes.
 * A third argument R repeats every SRS call R more times under the host clock and prints the per-call latency
 * (microseconds: median, min, max over all repeats) as one JSON line (tools/srs_rate.py).
 */
#define _POSIX_C_SOURCE 199309L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "srslte/srslte.h"

static int pusch(srslte_ue_ul_t *q, srslte_softbuffer_tx_t *sb, uint16_t rnti, uint8_t *payload, cf_t *signal) {
  srslte_ra_ul_grant_t grant;
  srslte_uci_data_t uci_data;
  memset(&grant, 0, sizeof(grant));
  memset(&uci_data, 0, sizeof(uci_data));
  grant.n_prb[0] = grant.n_prb[1] = 1;
  grant.L_prb = 3;
  grant.mcs.tbs = 256;
  grant.Qm = 2;
  if (srslte_ue_ul_cfg_grant(q, &grant, 9, 0, 0)) return -2;
  return srslte_ue_ul_pusch_encode_rnti_softbuffer(q, payload, uci_data, sb, rnti, signal) ? -3 : 0;
}

static int cmp_double(const void *a, const void *b) {
  const double x = *(const double *)a, y = *(const double *)b;
  return x < y ? -1 : x > y;
}

int main(int argc, char **argv) {
  if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s in.bin out.bin [repeats]\n", argv[0]); return 2; }
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
  srslte_ue_ul_set_normalization(&ue_ul, (hdr[6] & 1) != 0);
  srslte_ue_ul_set_cfo_enable(&ue_ul, (hdr[6] & 2) != 0);
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
  power_ctrl.p0_nominal_pusch = f[2];
  power_ctrl.alpha = f[3];
  power_ctrl.p0_nominal_pucch = f[4];
  for (int i = 0; i < 5; i++) power_ctrl.delta_f_pucch[i] = f[5 + i];
  power_ctrl.delta_preamble_msg3 = f[10];
  power_ctrl.p0_ue_pusch = f[11];
  power_ctrl.p0_ue_pucch = f[12];
  power_ctrl.p_srs_offset = f[13];
  power_ctrl.delta_mcs_based = hdr[18] != 0;
  power_ctrl.acc_enabled = hdr[19] != 0;
  srslte_ue_ul_set_cfg(&ue_ul, &dmrs_cfg, &srs_cfg, &pucch_cfg, &pucch_sched, &uci_cfg, &pusch_hopping, &power_ctrl);
  srslte_ue_ul_set_rnti(&ue_ul, (uint16_t)hdr[17]);
  srslte_softbuffer_tx_t softbuffer;
  if (srslte_softbuffer_tx_init(&softbuffer, 100)) { fprintf(stderr, "softbuffer_tx\n"); return 3; }
  const uint32_t sflen = SRSLTE_SF_LEN_PRB(cell.nof_prb);
  cf_t *signal = (cf_t *)srslte_vec_malloc(sflen * sizeof(cf_t));
  cf_t *before = (cf_t *)srslte_vec_malloc(sflen * sizeof(cf_t));
  uint8_t payload[32];
  for (int i = 0; i < 32; i++) payload[i] = (uint8_t)(37 * i + 11);
  int32_t pr[2] = {0, 0};
  const int reps = argc == 4 ? atoi(argv[3]) : 0;
  double *us = reps > 0 ? (double *)malloc(sizeof(double) * (size_t)reps * (size_t)(hdr[2] > 0 ? hdr[2] : 1)) : NULL;
  size_t n_us = 0;
  memset(before, 0, sflen * sizeof(cf_t));
  if (hdr[16]) pr[0] = pusch(&ue_ul, &softbuffer, (uint16_t)hdr[17], payload, before);
  for (int i = 0; i < hdr[2]; i++) {
    int32_t tti;
    if (fread(&tti, 4, 1, fi) != 1) return 4;
    srslte_ue_ul_set_cfo(&ue_ul, f[0]);
    memset(signal, 0, sflen * sizeof(cf_t));
    const int32_t ret = mi_ue_ul_srs_encode(&ue_ul, (uint32_t)tti, signal);
    const float tx_power = mi_ue_ul_srs_power(&ue_ul, f[1]);
    fwrite(&ret, 4, 1, fo);
    fwrite(&tx_power, 4, 1, fo);
    fwrite(signal, 8, sflen, fo);
    for (int k = 0; k < reps && !ret; k++) {
      struct timespec t0, t1;
      clock_gettime(CLOCK_MONOTONIC, &t0);
      if (mi_ue_ul_srs_encode(&ue_ul, (uint32_t)tti, signal)) return 5;
      clock_gettime(CLOCK_MONOTONIC, &t1);
      us[n_us++] = (double)(t1.tv_sec - t0.tv_sec) * 1e6 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-3;
    }
  }
  if (n_us) {
    qsort(us, n_us, sizeof(double), cmp_double);
    printf("{\"calls\": %zu, \"median_us\": %.2f, \"min_us\": %.2f, \"max_us\": %.2f}\n", n_us, us[n_us / 2], us[0],
           us[n_us - 1]);
  }
  free(us);
  float pw[9];
  pw[0] = mi_ue_ul_pusch_power(&ue_ul, f[1], 0.0f);
  pw[1] = mi_ue_ul_pusch_power(&ue_ul, f[1], f[14]);
  for (uint32_t fmt = 0; fmt < 6; fmt++) pw[2 + fmt] = mi_ue_ul_pucch_power(&ue_ul, f[1], fmt, 11, 1);
  pw[8] = mi_ue_ul_srs_power(&ue_ul, f[1]);
  fwrite(pw, 4, 9, fo);
  if (hdr[16]) {
    memset(signal, 0, sflen * sizeof(cf_t));
    pr[1] = pusch(&ue_ul, &softbuffer, (uint16_t)hdr[17], NULL, signal);
    fwrite(pr, 4, 2, fo);
    fwrite(before, 8, sflen, fo);
    fwrite(signal, 8, sflen, fo);
  }
  srslte_softbuffer_tx_free(&softbuffer);
  srslte_ue_ul_free(&ue_ul);
  srslte_vec_free(signal);
  srslte_vec_free(before);
  fclose(fi);
  fclose(fo);
  return 0;
}
