// prach.h -- shared host/device definitions and the host planner of the PRACH preamble transmitter (36.211 5.7;
// FDD, preamble formats 0-3, N_ZC = 839, unrestricted and restricted sets): what srsUE's prach.cc reaches through
// its preamble init / gen calls.  No HIP dependency: prach_host.cpp plans, prach.hip generates.
#pragma once
#include <vector>

#include "dl_common.h"
#include "mi_ul.h"

// one preamble transmission: CP + sequence (once for formats 0/1, twice for 2/3) at the UL sample rate 15 kHz N_ul
struct MiPrachTx {
  uint64_t iq_off;      // float2 offset of its first CP sample
  uint32_t N_ifft;      // 12 N_ul: the 1.25 kHz grid at the UL sample rate
  uint32_t N_ul;        // srslte_symbol_sz(nof_prb)
  uint32_t L;           // N_ifft / 1536: polyphase branches (1, 2, 4, 8, 12, 16)
  uint32_t N_cp, reps;  // CP samples; 1 or 2 copies of the sequence
  uint32_t root_slot;   // index of its root in the plan's list of distinct roots
  uint32_t C_v;         // cyclic shift
  uint32_t first_bin;   // bin of X(0) in the N_ifft-point grid
};
// one workgroup of prach_gen_kernel: residues r0 .. r0 + rpw - 1 of transmission tx
struct MiPrachItem {
  uint32_t tx, r0, rpw;   // rpw = 1, 2 or 4, a divisor of the transmission's L
};

namespace mi {
constexpr int PRACH_THREADS = 256;
constexpr uint32_t PRACH_NZC = 839;      // N_ZC of formats 0-3
constexpr uint32_t PRACH_NFFT = 1536;    // the LDS transform: 3 . 8 . 8 . 8
constexpr uint32_t PRACH_RPW_MAX = 4;    // residues a workgroup may own (1536-point results kept in LDS at once)

// the 64 preambles of a cell (5.7.2): physical root and cyclic shift of each, and how many roots they use
struct PrachCell {
  uint32_t u[64], C_v[64], n_roots;
};
// false + set_error when root / zero_corr_zone / high_speed are out of range or 838 roots give fewer than 64
bool prach_cell(uint32_t root_seq_idx, uint32_t zero_corr_zone, uint32_t high_speed, PrachCell* out);

struct PrachPlan {
  std::vector<MiPrachTx> txs;
  std::vector<mi_prach_res_t> res;
  std::vector<uint32_t> roots;        // distinct physical roots, one workgroup row of prach_root_kernel each
  std::vector<MiPrachItem> items;     // workgroups of prach_gen_kernel
  uint32_t rpw_cap = PRACH_RPW_MAX;   // 1 = the single-residue variant (MI_PRACH_FLAG_SINGLE_RESIDUE)
  size_t iq_samples = 0;
  int build(const mi_prach_cfg_t* cfgs, uint32_t n);   // 0 / -1 + set_error; nothing is kept of a rejected batch
};
}  // namespace mi
