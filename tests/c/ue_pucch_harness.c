/*
 * ue_pucch_harness.c -- drives mi_ue_ul_pucch_encode (include/srslte/srslte.h) the way srsUE's phch_worker drives
 * its PUCCH encode call (phch_worker.cc:597-629): init_cell as for PUSCH (srslte_ue_ul_init, _set_normalization,
 * _set_cfo_enable, _set_rnti, _set_cfg with the PUCCH configuration), then per TTI srslte_ue_ul_set_cfo and
 * mi_ue_ul_pucch_encode(&ue_ul, uci_data, n_cce, tti, signal), reading ue_ul.last_pucch_format and
 * ue_ul.pucch.shortened afterwards.
 * Input file : int32 hdr[16] = {cell_id, nof_prb, ncalls, group_hopping, flags (1 = normalisation, 2 = CFO),
 *              delta_pucch_shift, N_cs, n_rb_2, srs_configured, srs_cs_subf_cfg, srs_simul_ack, N_pucch_1, n_pucch_2,
 *              n_pucch_sr, rnti, pusch} + float cfo; per call int32 p[6] = {tti, n_cce, ack_len, ack, sr, cqi_len} +
 *              64 CQI bit bytes.  pusch = 1: one PUSCH subframe (3 PRB, 256 bits, QPSK) is encoded before the PUCCH
 *              calls, and again after them from the HARQ softbuffer (payload NULL).
 * Output file: per call int32 r[3] = {ret, last_pucch_format, pucch.shortened} + SF_LEN cf32 samples; with pusch = 1
 *              then int32 {ret before, ret after} + the two PUSCH subframes.
 * A third argument R repeats every PUCCH call R more times under the host clock and prints the per-call latency
 * (microseconds: median, min, max over all repeats) as one JSON line (tools/pucch_rate.py).
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
  if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  int32_t hdr[16];
  float cfo;
  if (fread(hdr, 4, 16, fi) != 16 || fread(&cfo, 4, 1, fi) != 1) return 2;
  srslte_cell_t cell;
  memset(&cell, 0, sizeof(cell));
  cell.id = (uint32_t)hdr[0];
  cell.nof_prb = (uint32_t)hdr[1];
  cell.nof_ports = 1;
  cell.cp = SRSLTE_CP_NORM;
  srslte_ue_ul_t ue_ul;
  if (srslte_ue_ul_init(&ue_ul, cell)) { fprintf(stderr, "ue_ul_init\n"); return 3; }
  srslte_ue_ul_set_normalization(&ue_ul, (hdr[4] & 1) != 0);
  srslte_ue_ul_set_cfo_enable(&ue_ul, (hdr[4] & 2) != 0);
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
  pucch_cfg.delta_pucch_shift = (uint32_t)hdr[5];
  pucch_cfg.N_cs = (uint32_t)hdr[6];
  pucch_cfg.n_rb_2 = (uint32_t)hdr[7];
  pucch_cfg.srs_configured = hdr[8] != 0;
  pucch_cfg.srs_cs_subf_cfg = (uint32_t)hdr[9];
  pucch_cfg.srs_simul_ack = hdr[10] != 0;
  pucch_sched.N_pucch_1 = (uint32_t)hdr[11];
  pucch_sched.n_pucch_2 = (uint32_t)hdr[12];
  pucch_sched.n_pucch_sr = (uint32_t)hdr[13];
  pusch_hopping.n_sb = 1;
  srslte_ue_ul_set_cfg(&ue_ul, &dmrs_cfg, &srs_cfg, &pucch_cfg, &pucch_sched, &uci_cfg, &pusch_hopping, &power_ctrl);
  srslte_ue_ul_set_rnti(&ue_ul, (uint16_t)hdr[14]);
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
  if (hdr[15]) pr[0] = pusch(&ue_ul, &softbuffer, (uint16_t)hdr[14], payload, before);
  for (int i = 0; i < hdr[2]; i++) {
    int32_t p[6];
    uint8_t cqi_bits[64];
    if (fread(p, 4, 6, fi) != 6 || fread(cqi_bits, 1, 64, fi) != 64) return 4;
    srslte_uci_data_t uci_data;
    memset(&uci_data, 0, sizeof(uci_data));
    uci_data.uci_ack_len = (uint32_t)p[2];
    uci_data.uci_ack = (uint8_t)p[3];
    uci_data.scheduling_request = p[4] != 0;
    uci_data.uci_cqi_len = (uint32_t)p[5];
    memcpy(uci_data.uci_cqi, cqi_bits, 64);
    srslte_ue_ul_set_cfo(&ue_ul, cfo);
    memset(signal, 0, sflen * sizeof(cf_t));
    ue_ul.last_pucch_format = 99;
    const int ret = mi_ue_ul_pucch_encode(&ue_ul, uci_data, (uint32_t)p[1], (uint32_t)p[0], signal);
    int32_t r[3] = {ret, (int32_t)ue_ul.last_pucch_format, (int32_t)ue_ul.pucch.shortened};
    fwrite(r, 4, 3, fo);
    fwrite(signal, 8, sflen, fo);
    for (int k = 0; k < reps && !ret; k++) {
      struct timespec t0, t1;
      clock_gettime(CLOCK_MONOTONIC, &t0);
      if (mi_ue_ul_pucch_encode(&ue_ul, uci_data, (uint32_t)p[1], (uint32_t)p[0], signal)) return 5;
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
  if (hdr[15]) {
    memset(signal, 0, sflen * sizeof(cf_t));
    pr[1] = pusch(&ue_ul, &softbuffer, (uint16_t)hdr[14], NULL, signal);
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
