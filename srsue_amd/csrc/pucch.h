// pucch.h -- shared host/device definitions and the host planner of the PUCCH transmitter (36.211 5.4,
// 5.5.2.2; formats 1/1a/1b and 2/2a/2b, normal CP): what srsUE reaches through the PUCCH encode call of its
// worker (srsUE phch_worker.cc:597-629).  No HIP dependency: pucch_host.cpp plans,
// pucch.hip encodes.
#pragma once
#include <vector>

#include "dl_common.h"
#include "mi_ul.h"

// one PUCCH transmission (one subframe of one UE); every RE it occupies is exp(j pi i / 12) for an integer i
struct MiPucchTx {
  uint64_t iq_off;       // float2 offset of its output subframe (15 N samples)
  uint32_t N, W;         // FFT size, 12 N_RB^UL
  uint32_t format;       // MI_PUCCH_*
  uint32_t shortened;    // formats 1x: slot 1 spreads over 3 data symbols, its last symbol is zeros
  uint32_t n_prb[2];     // PRB of slots 0 / 1
  uint32_t u[2];         // base-sequence group of slots 0 / 1
  uint32_t ncs[2];       // cyclic shifts n_cs(ns, l), 4 bits per symbol (l = 0 lowest)
  uint32_t n_oc[2];      // orthogonal-cover index (formats 1x)
  uint32_t s_odd[2];     // n'(ns) odd: S(ns) = j (formats 1x)
  uint32_t scr;          // formats 2x: scrambling bits c(0..19), c(i) at bit 31 - i (the layout of the code word)
  uint32_t cqi_len;      // formats 2x: A
  float scale;           // output amplitude factor (1; srslte_ue_ul_set_normalization)
  float cfo;             // frequency shift applied to the output, subcarriers (0; srslte_ue_ul_set_cfo)
};

namespace mi {
constexpr int PUCCH_THREADS = 256;
constexpr int PUCCH_NCOL = 11;    // columns of the (20, A) code available (36.212 Table 5.2.3.3-1, A <= 11)

struct PucchPlan {
  std::vector<MiPucchTx> txs;
  std::vector<mi_pucch_res_t> res;
  uint32_t rm[PUCCH_NCOL];        // (20, A) basis by columns: bit 31 - i of rm[n] = M_{i,n}, i < 20
  size_t iq_samples = 0;
  int build(const mi_pucch_cfg_t* cfgs, uint32_t n);   // 0 / -1 + set_error; nothing is kept of a rejected batch
};
}  // namespace mi
