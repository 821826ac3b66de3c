/*
 * ue_prach_harness.c -- drives the PRACH calls (include/srslte/srslte.h, include/mi_ul.h) the way srsUE's prach.cc
 * does: init_cell (prach.cc:77-98) = mi_prach_init with mi_prach_get_preamble_format(config_idx) and
 * srslte_symbol_sz(nof_prb), reading N_seq and N_cp, then 64 x mi_prach_gen; is_ready_to_send (:130) =
 * mi_prach_send_tti, swept over every config_idx and the ttis of two frames; send (:152,168) = mi_prach_gen_cfo;
 * the destructor = mi_prach_free.
 * Input file : int32 hdr[8] = {nof_prb, config_idx, root_seq_index, high_speed, zero_corr_zone, freq_offset,
 *              preamble of the gen_cfo call, 0} + float cfo (subcarriers) + float scale.
 * Output file: int32 {init ret, N_seq, N_cp}; if init failed nothing more.  Then 64 x (int32 ret + N_cp + N_seq cf32
 *              samples), 64 x 20 bytes of mi_prach_send_tti(config, tti, -1), int32 gen_cfo ret + its samples.
 * A third argument R times, under the host clock, init + 64 x gen on a fresh instance and R calls each of
 * mi_prach_gen (preambles already on the device) and mi_prach_gen_cfo, and prints one JSON line
 * (tools/prach_rate.py).
 */
#define _POSIX_C_SOURCE 199309L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "srslte/srslte.h"
#include "mi_ul.h"

static double now_us(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec * 1e6 + (double)t.tv_nsec * 1e-3;
}

static int cmp_double(const void *a, const void *b) {
  const double x = *(const double *)a, y = *(const double *)b;
  return x < y ? -1 : x > y;
}

int main(int argc, char **argv) {
  if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s in.bin out.bin [repeats]\n", argv[0]); return 2; }
  FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  int32_t hdr[8];
  float par[2];
  if (fread(hdr, 4, 8, fi) != 8 || fread(par, 4, 2, fi) != 2) return 2;
  const uint32_t N_ul = (uint32_t)srslte_symbol_sz((uint32_t)hdr[0]), freq_offset = (uint32_t)hdr[5];
  srslte_prach_t prach_obj;
  memset(&prach_obj, 0, sizeof(prach_obj));
  const int ret = mi_prach_init(&prach_obj, N_ul, mi_prach_get_preamble_format((uint32_t)hdr[1]), (uint32_t)hdr[2],
                                hdr[3] != 0, (uint32_t)hdr[4]);
  int32_t r3[3] = {ret, (int32_t)prach_obj.N_seq, (int32_t)prach_obj.N_cp};
  fwrite(r3, 4, 3, fo);
  if (ret) {
    fclose(fi);
    fclose(fo);
    return 0;
  }
  const uint32_t len = prach_obj.N_seq + prach_obj.N_cp;
  cf_t *signal = (cf_t *)srslte_vec_malloc(len * sizeof(cf_t));
  for (uint32_t i = 0; i < 64; i++) {
    memset(signal, 0, len * sizeof(cf_t));
    int32_t g = mi_prach_gen(&prach_obj, i, freq_offset, signal);
    fwrite(&g, 4, 1, fo);
    fwrite(signal, 8, len, fo);
  }
  for (uint32_t c = 0; c < 64; c++) {
    uint8_t row[20];
    for (uint32_t tti = 0; tti < 20; tti++) row[tti] = (uint8_t)mi_prach_send_tti(c, tti, -1);
    fwrite(row, 1, 20, fo);
  }
  memset(signal, 0, len * sizeof(cf_t));
  int32_t g = mi_prach_gen_cfo(&prach_obj, (uint32_t)hdr[6], freq_offset, par[0], par[1], signal);
  fwrite(&g, 4, 1, fo);
  fwrite(signal, 8, len, fo);
  const int reps = argc == 4 ? atoi(argv[3]) : 0;
  if (reps > 0 && !g) {
    double *us = (double *)malloc(sizeof(double) * (size_t)reps);
    double med[2];
    for (int which = 0; which < 2; which++) {
      for (int k = 0; k < reps; k++) {
        const double t0 = now_us();
        const int e = which ? mi_prach_gen_cfo(&prach_obj, (uint32_t)(k % 64), freq_offset, par[0], par[1], signal)
                            : mi_prach_gen(&prach_obj, (uint32_t)(k % 64), freq_offset, signal);
        us[k] = now_us() - t0;
        if (e) return 5;
      }
      qsort(us, (size_t)reps, sizeof(double), cmp_double);
      med[which] = us[reps / 2];
    }
    /* the cell set-up of init_cell on a fresh instance (the device and the code objects are warm by now) */
    srslte_prach_t fresh;
    memset(&fresh, 0, sizeof(fresh));
    const double t0 = now_us();
    if (mi_prach_init(&fresh, N_ul, mi_prach_get_preamble_format((uint32_t)hdr[1]), (uint32_t)hdr[2], hdr[3] != 0,
                      (uint32_t)hdr[4]))
      return 5;
    for (uint32_t i = 0; i < 64; i++)
      if (mi_prach_gen(&fresh, i, freq_offset, signal)) return 5;
    const double setup = now_us() - t0;
    mi_prach_free(&fresh);
    printf("{\"calls\": %d, \"gen_median_us\": %.2f, \"gen_cfo_median_us\": %.2f, \"init_64_gen_us\": %.1f}\n", reps,
           med[0], med[1], setup);
    free(us);
  }
  mi_prach_free(&prach_obj);
  srslte_vec_free(signal);
  fclose(fi);
  fclose(fo);
  return 0;
}
