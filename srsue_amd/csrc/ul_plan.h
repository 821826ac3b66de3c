// ul_plan.h -- host planner of the UL PUSCH transmit path (no HIP dependency): segmentation, rate
// matching splits and selection tables, scrambling words, DMRS parameters, DFT radix plans and
// twiddle tables for a batch of transmissions.
#pragma once
#include <array>
#include <map>
#include <vector>

#include "mi_ul.h"
#include "tables.h"
#include "ul_common.h"

namespace mi {

// 36.211 5.5.2.1 / 5.5.1: DMRS root q, Zadoff-Chu length and cyclic shift of slot ns (0..19)
int ul_dmrs_params(const mi_ul_cfg_t& c, uint32_t ns, uint32_t* q, uint32_t* nzc, uint32_t* ncs);
// 36.211 5.5.1.3: sequence-group number u = (f_gh(ns) [with group hopping] + f_ss) mod 30 of slot ns (0..19).  f_ss is
// the caller's: (N_ID + delta_ss) mod 30 for the PUSCH, N_ID mod 30 for the PUCCH and the SRS.  f_gh of the whole
// frame is kept per thread and cell
uint32_t ul_group_u(uint32_t cell_id, uint32_t ns, bool group_hopping, uint32_t fss);
// 36.211 5.5.1.4: the sequence-hopping bit c(ns), c_init = floor(N_ID / 30) 2^5 + f_ss^PUSCH, kept likewise
uint32_t ul_seq_hop_bit(uint32_t cell_id, uint32_t fss_pusch, uint32_t ns);
// 36.211 5.5.1.1 / 5.5.1.2: root q and Zadoff-Chu length of the base sequence r_{u,v} of length M (a multiple of
// 12); M < 36: the tabulated sequences, nzc = 0 and q = u.  Shared by the PUSCH DMRS and the SRS (srs_host.cpp)
void ul_base_seq(uint32_t M, uint32_t u, uint32_t v, uint32_t* q, uint32_t* nzc);
// radix list (8, 4, 2, 3, 5; 4 bits per stage) of an n-point transform, 0 if n has another factor
uint32_t ul_radix_plan(uint32_t n);
// CQI channel coding on PUSCH (36.212 5.2.2.6.4): the Q coded bits of the O-bit report o (O <= 11: the
// (32, O) block code repeated; O > 11: CRC8, tail-biting convolutional code, 5.1.4.2 rate matching)
void ul_cqi_code(const uint8_t* o, uint32_t O, uint32_t Q, std::vector<uint8_t>& q);

// every check and the 36.212 5.2.2.6 arithmetic of one transmission (mi_ul_pusch_resource; UlPlan::build plans
// through it): 0 with *sg and *r filled, or -1 + set_error with *r untouched
int ul_pusch_resource(const mi_ul_cfg_t& c, CbSegm* sg, mi_ul_res_t* r);

struct UlPlan {
  std::vector<MiUlTx> txs;
  std::vector<MiUlCb> cbs;
  std::vector<uint32_t> kdata;      // QPP and selection tables
  std::vector<uint32_t> scr;        // scrambling words
  std::vector<float> tw;            // float2 twiddle tables
  std::vector<uint32_t> tb_cb0;     // first code block of each transmission (n + 1 entries)
  std::vector<uint8_t> cqi_syms;    // CQI coded symbols of every transmission (Qm bits per byte, MSB first)
  std::vector<uint32_t> cqi_off;    // per transmission: offset of its Q'_CQI symbols in cqi_syms
  size_t payload_bytes = 0, sym_bytes = 0, iq_samples = 0;
  double algo_bytes = 0;

  std::map<uint32_t, uint32_t> pi_off, tw_off;
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> sel_off;   // (K, F) -> kdata offset of this build
  // per-key tables kept across builds (the per-TTI path re-plans every grant)
  struct SelTab { std::vector<uint32_t> sel; uint32_t r0[4]; };
  std::map<std::pair<uint32_t, uint32_t>, SelTab> sel_cache;
  std::map<uint32_t, std::vector<uint32_t>> pi_cache;
  std::map<uint32_t, std::vector<float>> tw_cache;   // DFT length -> interleaved cos / sin twiddles
  // scrambling words by (c_init, bits): srsUE's RNTI and cell are fixed, so a worker sees a handful of
  // keys (10 subframes x the grant sizes); bounded, cleared when it grows past SCR_CACHE_MAX
  std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> scr_cache;
  static constexpr size_t SCR_CACHE_MAX = 256;
  int build(const mi_ul_cfg_t* cfgs, uint32_t n);
};

}  // namespace mi
