// srs.h -- shared host/device definitions and the host planner of the SRS transmitter (36.211 5.5.3, periodic SRS,
// FDD, normal CP): what srsUE reaches through the SRS encode call of its worker (srsUE phch_worker.cc:636-656).
// No HIP dependency: srs_host.cpp plans, srs.hip encodes.
#pragma once
#include <vector>

#include "dl_common.h"
#include "mi_ul.h"

// one SRS transmission (one subframe of one UE): a_{k0 + 2 k'} = exp(j 2 pi n_cs k' / 8) rbar_{u,v}(k') in symbol 13
struct MiSrsTx {
  uint64_t iq_off;       // float2 offset of its output subframe (15 N samples)
  uint32_t N;            // FFT size; the transform runs on N / 2 points
  uint32_t M_sc;         // sequence length, 24 .. 576, <= N / 2
  int32_t K;             // k0 - 6 N_RB^UL: first subcarrier relative to the band centre
  uint32_t nzc, q;       // Zadoff-Chu length and root; nzc = 0: tabulated M_sc = 24 sequence of group q
  uint32_t n_cs;         // cyclic shift 0..7
  float scale;           // output amplitude factor (1; srslte_ue_ul_set_normalization)
  float cfo;             // frequency shift applied to the output, subcarriers (0; srslte_ue_ul_set_cfo)
};

namespace mi {
constexpr int SRS_THREADS = 256;
constexpr int SRS_HMAX = 1024;     // the largest half-length transform (N = 2048): 8 KiB of LDS
constexpr int SRS_ZERO_PARTS = 7;  // workgroups per transmission that write the zeros of symbols 0..12

// 36.213 Table 8.2-1 (FDD), held by srslte_util.cpp: 0, or -1 for a reserved I_SRS
int srs_ue_period(uint32_t I_srs, uint32_t* T_srs, uint32_t* T_offset);

struct SrsPlan {
  std::vector<MiSrsTx> txs;
  std::vector<mi_srs_res_t> res;
  size_t iq_samples = 0;
  int build(const mi_srs_cfg_t* cfgs, uint32_t n);   // 0 / -1 + set_error; nothing is kept of a rejected batch
};
}  // namespace mi
